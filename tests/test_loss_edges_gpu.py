"""losses.hip at the class counts and grid caps test_losses_gpu.py never reaches, against float64: oracle/losses.py
evaluated in float64 (through tests/fp64_refs.py) and the numpy Dice of oracle/metrics.py.

case -> branch
  seg_loss C = 1, 2, 3, 6, 7, 8 x mode          every flat-walk seg_partial_kernel<C> the existing tests (C = 4, 5) leave out
  seg_loss (1, 1), (2, 257)                     one pixel; one ragged block; +-40 logits: the BCE log clamp and its backward
  seg_loss (1, 2, 513 * 512)                    262656 pixels: SEG_BLOCKS = 1024 caps the grid, two trips per thread
  seg_loss (1, 2, 1025 * 1024)                  1049600 pixels: the backward's 4096-block cap, two trips per thread
  seg_loss (4100, 3, 3)                         more samples than either pass's block budget: one block per sample
  seg_loss C = 9, entropy C = 17, nn_loss 1025  refused before any launch
  entropy C = 1, 2, 16 x mode x norm            the per-pixel channel loops at their ends (MAXC = 16)
  entropy_bwd accumulate / dmean / all three    the `+=`, the mean's share alone, every source together
  entropy (1, 2, 1025 * 1024)                   1049600 pixels: grid_for's 4096-block cap
  jaccard C = 1, 16, uint8 / float truth        both truth readers; gout NULL and given
  jaccard (1, 3, 257 * 256)                     65792 pixels: JAC_BLOCKS = 256 caps the grid
  bce_const 1, 255, 257, 5000                   one workgroup striding over the input; labels 0 / 1; gscale; accuracy
  sum_all 1, 1023, 1025, 524288 + 5             one block, two blocks, SUM_BLOCKS = 512 capped; scale
  dice_metric (1, 4, 513 * 512)                 the count kernel's 1024-block cap
  argmax_labels / dice_metric, NaN and +-inf    np.max propagates NaN: label 0, no channel counted; -0.0 == +0.0 ties

Bounds: scalars within 1e-5 * max(1, |ref|); loss gradients 1e-4 (2e-4 where logits are saturated, as
test_losses_against_oracle_large allows); entropy maps and probabilities 1e-5 (the project's bound for them);
accuracy and Dice 1e-6.
"""
import math

import numpy as np
import pytest
import torch

import fp64_refs as R
from conftest import rel_err

pytestmark = pytest.mark.gpu


def _rand(rng, *shape, scale=1.0):
    return torch.from_numpy(rng.normal(0, scale, shape).astype(np.float32))


def _close(got, ref, tol=1e-5):
    return abs(float(got) - float(ref)) < tol * max(1.0, abs(float(ref)))


def _onehot(rng, n, c, hw):
    if c == 1:
        return torch.from_numpy(rng.integers(0, 2, (n, 1, hw)).astype(np.uint8))
    lab = rng.integers(0, c, (n, hw))
    return torch.from_numpy(np.moveaxis(np.eye(c, dtype=np.uint8)[lab], -1, 1).copy())


SEG = [(c, n, hw) for c in (1, 2, 3, 6, 7, 8) for (n, hw) in ((1, 1), (2, 257))] + [(2, 1, 513 * 512), (2, 1, 1025 * 1024),
                                                                                     (3, 4100, 3)]


@pytest.mark.parametrize("mode", ["sigmoid", "softmax"])
@pytest.mark.parametrize("c,n,hw", SEG, ids=["C%d-%dx%d" % s for s in SEG])
def test_seg_loss_every_class_count(dev, c, n, hw, mode):
    from pointcloududa_amd import kernels as K
    rng = np.random.default_rng(10 * c + n + hw)
    logits = _rand(rng, n, c, hw, scale=2.0)
    saturated = hw >= 8
    if saturated:
        logits[0, 0, :4] = 40.0
        logits[0, c - 1, 4:8] = -40.0
    onehot = _onehot(rng, n, c, hw)
    main_r, jac_r, grad_r = R.seg_loss(logits, onehot, mode, 1.0, 0.7)
    ld, od = logits.to(dev), onehot.to(dev)
    out2, ws = K.seg_loss_fwd(ld, od, mode)
    grad = K.seg_loss_bwd(ld, od, mode, ws, None, torch.full((), 0.7, device=dev))
    print("seg_loss C=%d %s: main %.8g (ref %.8g) jac %.8g (ref %.8g) grad %.3g" % (
        c, mode, float(out2[0]), float(main_r), float(out2[1]), float(jac_r), rel_err(grad, grad_r)))
    assert _close(out2[0], main_r) and _close(out2[1], jac_r)
    assert rel_err(grad, grad_r) < (2e-4 if saturated else 1e-4)


def test_class_and_point_counts_past_the_limits_raise(dev):
    from pointcloududa_amd import kernels as K
    with pytest.raises(RuntimeError):
        K.seg_loss_fwd(torch.zeros(1, 9, 16, device=dev), torch.zeros(1, 9, 16, dtype=torch.uint8, device=dev), "sigmoid")
    with pytest.raises(RuntimeError):
        K.entropy_fwd(torch.zeros(1, 17, 16, device=dev), "softmax")
    with pytest.raises(RuntimeError):
        K.entropy_bwd(torch.zeros(1, 17, 16, device=dev), "softmax", 1.0, dent=torch.zeros(1, 17, 16, device=dev))
    with pytest.raises(RuntimeError):
        K.nn_loss_fwd(torch.zeros(1, 1025, 3, device=dev), torch.zeros(1, 1025, 3, device=dev))


ENT = [(2, 1, 257), (2, 2, 257), (2, 16, 257)]


def _norm(c, on):
    """1 / log C as train_mmwhs.py normalises (C = 1, where that is undefined: another multiplier that is not 1)"""
    return (1.0 / math.log(c) if c > 1 else 0.75) if on else 1.0


# (the grid cap does not depend on the multiplier: the large case runs with one)
ENT_CASES = [s + (on,) for s in ENT for on in (False, True)] + [(1, 2, 1025 * 1024, True)]


@pytest.mark.parametrize("mode", ["sigmoid", "softmax"])
@pytest.mark.parametrize("n,c,hw,norm_on", ENT_CASES, ids=["C%d-%d-norm%d" % (s[1], s[2], s[3]) for s in ENT_CASES])
def test_entropy_maps_and_their_backward(dev, n, c, hw, norm_on, mode):
    from pointcloududa_amd import kernels as K
    big = hw > 1000
    rng = np.random.default_rng(100 * c + hw % 97)
    norm = _norm(c, norm_on)
    logits = _rand(rng, n, c, hw, scale=2.0)
    ld = logits.to(dev)
    ent_r, prob_r = R.entropy(logits, mode, norm)
    ent, prob = K.entropy_fwd(ld, mode, norm, want_prob=True)
    ent_only, none = K.entropy_fwd(ld, mode, norm)
    assert none is None and torch.equal(ent_only, ent)
    print("entropy C=%d %s: ent %.3g prob %.3g" % (c, mode, rel_err(ent, ent_r), rel_err(prob, prob_r)))
    assert rel_err(prob, prob_r) < 1e-5
    if mode == "softmax" and c == 1:
        # p = 1 everywhere: the map is -log(1 + 1e-7) * norm ~ -1e-7 in EVERY element, and float32 cannot hold 1 + 1e-7
        # (it rounds to 1 + 2^-23: log gives 1.19e-7).  float32 torch on the CPU is 0.192 off float64 here; four times that
        # is allowed.  The figure the kernel gives is printed above.
        assert rel_err(ent, ent_r) < 4 * 0.192
    else:
        assert rel_err(ent, ent_r) < 1e-5
    w1, w2 = _rand(rng, n, c, hw), _rand(rng, n, c, hw)
    dm = torch.tensor(0.3 * n * hw, dtype=torch.float32)          # (so that the mean's share is of the size of the others)
    w1d, w2d, dmd = w1.to(dev), w2.to(dev), dm.to(dev)
    g_all = K.entropy_bwd(ld, mode, norm, dent=w1d, dprob=w2d, dmean=dmd)
    assert rel_err(g_all, R.entropy_backward(logits, mode, norm, w1, w2, dm)) < 1e-4
    if big:
        return
    pre = _rand(rng, n, c, hw)
    out = pre.to(dev)
    K.entropy_bwd(ld, mode, norm, dent=w1d, out=out, accumulate=True)
    assert rel_err(out, pre.double() + R.entropy_backward(logits, mode, norm, w1)) < 1e-4
    assert rel_err(K.entropy_bwd(ld, mode, norm, dmean=dmd), R.entropy_backward(logits, mode, norm, dmean=dm)) < 1e-4
    assert rel_err(K.entropy_bwd(ld, mode, norm, dprob=w2d), R.entropy_backward(logits, mode, norm, dprob=w2)) < 1e-4


JAC = [(2, 1, 257), (2, 16, 257), (1, 3, 257 * 256)]


@pytest.mark.parametrize("with_gout", [False, True])
@pytest.mark.parametrize("u8", [True, False])
@pytest.mark.parametrize("n,c,hw", JAC, ids=["C1", "C16", "C3-257x256"])
def test_jaccard_on_given_probabilities(dev, n, c, hw, u8, with_gout):
    from pointcloududa_amd import kernels as K
    rng = np.random.default_rng(7 * c + u8)
    logits = _rand(rng, n, c, hw, scale=2.0)
    probs = torch.sigmoid(logits) if c == 1 else torch.softmax(logits, 1)
    truth = _onehot(rng, n, c, hw) if u8 else torch.from_numpy(rng.random((n, c, hw), dtype=np.float32))
    gout = 0.7 if with_gout else 1.0
    loss_r, grad_r = R.jaccard(truth, probs, 1e-7, gout)
    loss, ws, td = K.jaccard_fwd(probs.to(dev), truth.to(dev), 1e-7)
    grad = K.jaccard_bwd(td, probs.shape, 1e-7, ws, torch.full((), 0.7, device=dev) if with_gout else None)
    print("jaccard C=%d: loss %.8g (ref %.8g) grad %.3g" % (c, float(loss), float(loss_r), rel_err(grad, grad_r)))
    assert _close(loss, loss_r)
    assert rel_err(grad, grad_r) < 1e-4


@pytest.mark.parametrize("label", [0.0, 1.0])
@pytest.mark.parametrize("numel", [1, 255, 257, 5000])
def test_bce_against_a_constant(dev, numel, label):
    from pointcloududa_amd import kernels as K
    rng = np.random.default_rng(numel)
    x = _rand(rng, numel, scale=2.0)
    xd = x.to(dev)
    loss_r, grad_r, acc_r = R.bce_const(x, label, gout=0.7, gscale=0.5)
    loss, acc = K.bce_const_fwd(xd, label, want_acc=True)
    loss2, none = K.bce_const_fwd(xd, label)
    assert none is None and float(loss2) == float(loss)
    assert _close(loss, loss_r) and abs(float(acc) - float(acc_r)) < 1e-6
    assert rel_err(K.bce_const_bwd(xd, label, torch.full((), 0.7, device=dev), gscale=0.5), grad_r) < 1e-4
    assert rel_err(K.bce_const_bwd(xd, label, None, gscale=0.5), grad_r / 0.7) < 1e-4
    assert rel_err(K.bce_const_bwd(xd, label, None), grad_r / 0.35) < 1e-4


@pytest.mark.parametrize("numel", [1, 1023, 1025, 524288 + 5])
def test_sum_all(dev, numel):
    from pointcloududa_amd import kernels as K
    x = _rand(np.random.default_rng(numel), numel) + 0.5
    ref = float(x.double().sum())
    assert _close(K.sum_all(x.to(dev)), ref)
    assert _close(K.sum_all(x.to(dev), scale=0.25), 0.25 * ref)


def test_dice_metric_past_the_block_cap(dev):
    from oracle import metrics as OM
    from pointcloududa_amd import kernels as K
    rng = np.random.default_rng(5)
    n, c, hw = 1, 4, 513 * 512
    logits = _rand(rng, n, c, hw, scale=2.0)
    onehot = _onehot(rng, n, c, hw)
    ref = OM.dice_coef_multilabel(onehot.numpy(), OM.soft_to_hard_pred(logits.numpy(), 1), c)
    assert abs(float(K.dice_metric(logits.to(dev), onehot.to(dev))) - ref) < 1e-6


def _nan_logits():
    """[2, 4, 9, 11] logits with non-finite pixels, as (logits, {pixel: expected label}): np.max propagates NaN, so the
    reference's soft_to_hard_pred marks no channel of a pixel that holds one, and its argmax gives 0"""
    rng = np.random.default_rng(77)
    x = rng.normal(0, 1, (2, 4, 9, 11)).astype(np.float32)
    nan, inf = np.float32(np.nan), np.float32(np.inf)
    px = {(0, 0, 0): ([nan, 0.3, 2.0, 1.0], 0),            # NaN in channel 0
          (0, 0, 1): ([0.1, nan, 0.5, 0.2], 0),            # in a middle channel, before the largest finite value
          (0, 3, 4): ([0.1, 0.7, nan, 0.2], 0),            # in a middle channel, after it
          (0, 8, 10): ([1.0, 2.0, 3.0, nan], 0),           # in the last channel
          (1, 0, 0): ([0.0, 1.0, 2.0, nan], 0),
          (1, 4, 5): ([nan, nan, nan, nan], 0),            # all NaN
          (1, 8, 10): ([nan, inf, 0.0, -inf], 0),          # NaN beside +inf
          (0, 1, 1): ([0.0, 1.0, 2.0, inf], 3),
          (0, 2, 2): ([-inf, -1.0, -3.0, -2.0], 1),
          (0, 5, 5): ([-inf, -inf, -inf, -inf], 0),        # a four-way tie
          (1, 2, 3): ([1.0, inf, inf, 0.0], 1),            # a tie at +inf: the first
          (1, 3, 3): ([-1.0, -0.0, 0.0, -2.0], 1),         # -0.0 == +0.0: a tie, the first
          (1, 3, 4): ([-1.0, 0.0, -0.0, -2.0], 1),
          (1, 6, 7): ([0.0, -0.0, -1.0, -1.0], 0)}
    for (n, i, j), (v, _) in px.items():
        x[n, :, i, j] = v
    return x, {k: lab for k, (_, lab) in px.items()}


def test_argmax_labels_with_nan_and_infinite_logits(dev):
    from oracle import metrics as OM
    from pointcloududa_amd import kernels as K
    x, labels = _nan_logits()
    ref = OM.argmax_labels(x)
    for (n, i, j), lab in labels.items():
        assert ref[n, i, j] == lab, (n, i, j)                            # the reference itself
    got = K.argmax_labels(torch.from_numpy(x).to(dev))
    assert got.dtype == torch.uint8 and np.array_equal(got.cpu().numpy(), ref)
    view = torch.from_numpy(np.ascontiguousarray(np.concatenate([x, x], 1))).to(dev)[:, 4:]     # batch stride 8 channels
    assert np.array_equal(K.argmax_labels(view).cpu().numpy(), ref)
    rng = np.random.default_rng(78)
    onehot = np.moveaxis(np.eye(4, dtype=np.uint8)[rng.integers(0, 4, (2, 9, 11))], -1, 1).copy()
    got8 = K.argmax_labels(torch.from_numpy(onehot).to(dev))              # the uint8 reader: unchanged
    assert np.array_equal(got8.cpu().numpy(), OM.argmax_labels(onehot))


def test_dice_metric_with_nan_and_infinite_logits(dev):
    from oracle import metrics as OM
    from pointcloududa_amd import kernels as K
    x, labels = _nan_logits()
    lab = np.random.default_rng(79).integers(0, 4, (2, 9, 11))
    for n, i, j in labels:
        lab[n, i, j] = 1 + (i + j) % 3                                   # foreground truth under every special pixel
    onehot = np.moveaxis(np.eye(4, dtype=np.uint8)[lab], -1, 1).copy()
    hard = OM.soft_to_hard_pred(x, 1)
    assert not hard[0, :, 0, 1].any() and not hard[1, :, 4, 5].any() and hard[0, :, 5, 5].all()
    assert hard[1, :, 3, 3].tolist() == [0, 1, 1, 0]
    ref = OM.dice_coef_multilabel(onehot, hard, 4)
    got = float(K.dice_metric(torch.from_numpy(x).to(dev), torch.from_numpy(onehot).to(dev)))
    assert abs(got - ref) < 1e-6, (got, ref)
    dropped = np.where(np.isnan(x), -np.inf, x)                         # what dropping the NaN would count: far outside
    assert abs(OM.dice_coef_multilabel(onehot, OM.soft_to_hard_pred(dropped, 1), 4) - ref) > 1e-3
