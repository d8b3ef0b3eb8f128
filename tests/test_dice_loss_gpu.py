"""csrc/dice_loss.hip and what is built on it (utils/loss.py, the train step's ``dice`` switch, validation) against the
float64 statements of tests/dice_refs.py.

case -> branch
  fused C = 1, 2, 3, 4, 5, 8 x mode x reduction    every seg_partial_kernel<C, true, *> in use; both reduce chains
  fused (1, 1), (2, 257), (3, 300)                 one pixel; one ragged block; several samples in one launch
  fused (1, 2, 513 * 512)                          262656 pixels: 1024 blocks cap the grid, two trips per thread
  +-40 logits in the first sample                  the BCE log clamp and its backward next to the Dice term
  seeds NULL / g_ov = 0.7; C = 9                   both seed readers; refused before any launch
  N = 65537, C = 1, hw = 3                         more samples than a grid's y axis holds
  one sample all background, one all foreground    a partial row that mixed samples could not pass
  dice_loss C = 1, 16, u8 / fp32, (1, 3, 257*256)  the paired branch, the class limit, both truth readers, the block cap
  DiceLoss u8 / int64, C = 2, 5, 16                the label readers; labels outside [0, C) counted, ignored, raised
  jaccard default; second runs                     the unchanged path bit for bit; every new call equals its repetition
  train step / epoch / valid_batch                 the switch through the callers

Bounds (those of tests/test_loss_edges_gpu.py for this family): scalars within 1e-5 * max(1, |ref|); gradients
rel_err < 1e-4, 2e-4 where logits are saturated at +-40."""
import functools
import types

import numpy as np
import pytest
import torch

import dice_refs as D
from conftest import rel_err

pytestmark = pytest.mark.gpu

OVERLAP = {"class": "dice", "sample": "dice_sample"}
EPS = {"class": 1e-7, "sample": 1e-6}


def _close(got, ref, tol=1e-5):
    return abs(float(got) - float(ref)) < tol * max(1.0, abs(float(ref)))


def _rand(rng, *shape, scale=1.0):
    return torch.from_numpy(rng.normal(0, scale, shape).astype(np.float32))


def _onehot(rng, n, c, hw):
    if c == 1:
        return torch.from_numpy(rng.integers(0, 2, (n, 1, hw)).astype(np.uint8))
    lab = rng.integers(0, c, (n, hw))
    return torch.from_numpy(np.moveaxis(np.eye(c, dtype=np.uint8)[lab], -1, 1).copy())


@functools.lru_cache(maxsize=None)
def _fused_inputs(c, n, hw):
    """(logits, onehot, saturated) of a fused case, shared by its modes and reductions and never written"""
    rng = np.random.default_rng(10 * c + n + hw)
    logits = _rand(rng, n, c, hw, scale=2.0)
    saturated = hw >= 8
    if saturated:
        logits[0, 0, :4] = 40.0
        logits[0, c - 1, 4:8] = -40.0
    return logits, _onehot(rng, n, c, hw), saturated


FUSED = [(c, n, hw) for c in (1, 2, 3, 4, 5, 8) for (n, hw) in ((1, 1), (2, 257), (3, 300))] + [(2, 1, 513 * 512)]


@pytest.mark.parametrize("reduce", ["class", "sample"])
@pytest.mark.parametrize("mode", ["sigmoid", "softmax"])
@pytest.mark.parametrize("c,n,hw", FUSED, ids=["C%d-%dx%d" % s for s in FUSED])
def test_fused_seg_loss_with_a_dice_term(dev, c, n, hw, mode, reduce):
    from pointcloududa_amd import kernels as K
    logits, onehot, saturated = _fused_inputs(c, n, hw)
    main_r, dice_r, grad_r = D.seg_loss_dice(logits, onehot, mode, reduce, EPS[reduce], 1.0, 0.7)
    grad_r1 = D.seg_loss_dice(logits, onehot, mode, reduce, EPS[reduce], 1.0, 1.0)[2]
    ld, od = logits.to(dev), onehot.to(dev)
    out2, ws = K.seg_loss_ov_fwd(ld, od, mode, OVERLAP[reduce], EPS[reduce])
    grad = K.seg_loss_ov_bwd(ld, od, mode, OVERLAP[reduce], ws, None, torch.full((), 0.7, device=dev))
    grad1 = K.seg_loss_ov_bwd(ld, od, mode, OVERLAP[reduce], ws, None, None)
    print("seg_loss_ov C=%d %s %s: main %.8g (ref %.8g) dice %.8g (ref %.8g) grad %.3g / %.3g" % (
        c, mode, reduce, float(out2[0]), float(main_r), float(out2[1]), float(dice_r), rel_err(grad, grad_r),
        rel_err(grad1, grad_r1)))
    assert _close(out2[0], main_r) and _close(out2[1], dice_r)
    tol = 2e-4 if saturated else 1e-4
    assert rel_err(grad, grad_r) < tol and rel_err(grad1, grad_r1) < tol
    # the same bits from a second run (no floating-point atomics, fixed reduce order)
    out2b, wsb = K.seg_loss_ov_fwd(ld, od, mode, OVERLAP[reduce], EPS[reduce])
    assert torch.equal(out2b, out2)
    assert torch.equal(K.seg_loss_ov_bwd(ld, od, mode, OVERLAP[reduce], wsb, None, None), grad1)


def test_fused_form_refuses_nine_classes(dev):
    from pointcloududa_amd import kernels as K
    from pointcloududa_amd.utils import loss as L
    l, y = torch.zeros(1, 9, 16, device=dev), torch.zeros(1, 9, 16, dtype=torch.uint8, device=dev)
    for ov in ("dice", "dice_sample"):
        with pytest.raises(RuntimeError):
            K.seg_loss_ov_fwd(l, y, "sigmoid", ov)
        with pytest.raises(RuntimeError):
            L.seg_loss(l, y, "softmax", ov)


def test_per_sample_with_more_samples_than_a_grid_y_axis(dev):
    """N = 65537 > 65535: the (sample, chunk) pairs lie on the x axis"""
    from pointcloududa_amd import kernels as K
    n, c, hw = 65537, 1, 3
    rng = np.random.default_rng(65537)
    logits, onehot = _rand(rng, n, c, hw, scale=2.0), _onehot(rng, n, c, hw)
    main_r, dice_r, grad_r = D.seg_loss_dice(logits, onehot, "sigmoid", "sample", 1e-6, 1.0, 0.7)
    ld, od = logits.to(dev), onehot.to(dev)
    out2, ws = K.seg_loss_ov_fwd(ld, od, "sigmoid", "dice_sample", 1e-6)
    grad = K.seg_loss_ov_bwd(ld, od, "sigmoid", "dice_sample", ws, None, torch.full((), 0.7, device=dev))
    print("N=65537 fused: main %.8g (ref %.8g) dice %.8g (ref %.8g) grad %.3g" % (
        float(out2[0]), float(main_r), float(out2[1]), float(dice_r), rel_err(grad, grad_r)))
    assert _close(out2[0], main_r) and _close(out2[1], dice_r)
    assert rel_err(grad, grad_r) < 1e-4
    # the stand-alone form on the same batch (its probabilities), and the label-map form (two classes)
    probs = torch.sigmoid(logits)
    loss_r, gp_r = D.dice_probs(onehot, probs, 1e-6, "sample")
    loss, ws2, td = K.dice_fwd(probs.to(dev), od, 1e-6, "sample")
    assert _close(loss, loss_r) and rel_err(K.dice_bwd(td, probs.shape, "sample", ws2, None), gp_r) < 1e-4
    l2 = _rand(rng, n, 2, hw, scale=2.0)
    lab = torch.from_numpy(rng.integers(0, 2, (n, hw)).astype(np.uint8))
    loss_r, gl_r, _ = D.dice_labels(l2, lab, 1e-6)
    loss, ws3, labd, bad = K.dice_labels_fwd(l2.to(dev), lab.to(dev), 1e-6)
    assert _close(loss, loss_r) and int(bad) == 0
    assert rel_err(K.dice_labels_bwd(l2.to(dev), labd, ws3, None), gl_r) < 1e-4


@pytest.mark.parametrize("mode", ["sigmoid", "softmax"])
def test_samples_that_differ_strongly_do_not_mix(dev, mode):
    """sample 0 is all background and predicted so; sample 1 is predicted as nothing (both logits low) and is all
    foreground (sigmoid mode) or foreground on one half and of no class on the other (softmax mode: with a softmax and a
    valid one-hot every S_n is 2 hw, and then the per-sample loss and the pooled one are the same function).  The samples'
    sums differ, so sums that mixed them in a partial row give another loss and another gradient: the pooled value -- the
    batch as ONE sample -- is computed below and is far from the reference.  (Logits of +-2, and some truth in every
    sample: where the truth of a whole sample is empty the softmax Jacobian cancels the gradient to zero, and a float32
    kernel is compared with rounding noise.)"""
    from pointcloududa_amd import kernels as K
    n, c, hw = 2, 2, 300                       # two blocks per sample
    rng = np.random.default_rng(300)
    logits = _rand(rng, n, c, hw, scale=0.1)
    logits[0, 0] += 2.0; logits[0, 1] -= 2.0
    logits[1] -= 2.0
    onehot = torch.zeros(n, c, hw, dtype=torch.uint8)
    onehot[0, 0] = 1
    onehot[1, 1, :(hw if mode == "sigmoid" else hw // 2)] = 1
    dice_r, grad_r = D.dice_autograd(logits, onehot, mode, "sample", 1e-6)
    l = logits.double().requires_grad_(True)
    pooled = D.dice_value(D.activate(l, mode).reshape(1, n * c, hw), onehot.double().reshape(1, n * c, hw), 1e-6, "sample")
    pooled.backward()
    assert rel_err(l.grad, grad_r) > 1e-1 and abs(float(pooled.detach()) - float(dice_r)) > 1e-2
    ld, od = logits.to(dev), onehot.to(dev)
    out2, ws = K.seg_loss_ov_fwd(ld, od, mode, "dice_sample", 1e-6)
    grad = K.seg_loss_ov_bwd(ld, od, mode, "dice_sample", ws, torch.zeros((), device=dev), None)      # the Dice term alone
    print("differing samples %s: dice %.8g (ref %.8g, pooled %.8g) grad %.3g" % (
        mode, float(out2[1]), float(dice_r), float(pooled.detach()), rel_err(grad, grad_r)))
    assert _close(out2[1], dice_r) and rel_err(grad, grad_r) < 1e-4
    probs = D.activate(logits.double(), mode).float()
    loss_r, gp_r = D.dice_probs(onehot, probs, 1e-6, "sample")
    loss, ws2, td = K.dice_fwd(probs.to(dev), od, 1e-6, "sample")
    assert _close(loss, loss_r) and rel_err(K.dice_bwd(td, probs.shape, "sample", ws2, None), gp_r) < 1e-4
    if mode == "softmax":        # the label-map form of the same batch: sample 1's labels name no class
        lab = torch.zeros(n, hw, dtype=torch.uint8)
        lab[1, :hw // 2], lab[1, hw // 2:] = 1, 255
        loss_r, gl_r, nbad = D.dice_labels(logits, lab, 1e-6)
        assert nbad == hw - hw // 2 and abs(float(loss_r) - float(dice_r)) < 1e-12
        loss, ws3, labd, bad = K.dice_labels_fwd(ld, lab.to(dev), 1e-6)
        assert _close(loss, loss_r) and int(bad) == nbad
        assert rel_err(K.dice_labels_bwd(ld, labd, ws3, None), gl_r) < 1e-4


PROBS = [(2, 1, 257), (2, 16, 257), (1, 3, 257 * 256)]


@pytest.mark.parametrize("reduce", ["class", "sample"])
@pytest.mark.parametrize("u8", [True, False])
@pytest.mark.parametrize("n,c,hw", PROBS, ids=["C1", "C16", "C3-257x256"])
def test_dice_on_given_probabilities(dev, n, c, hw, u8, reduce):
    from pointcloududa_amd import kernels as K
    rng = np.random.default_rng(7 * c + u8)
    logits = _rand(rng, n, c, hw, scale=2.0)
    probs = torch.sigmoid(logits) if c == 1 else torch.softmax(logits, 1)
    truth = _onehot(rng, n, c, hw) if u8 else torch.from_numpy(rng.random((n, c, hw), dtype=np.float32))
    loss_r, grad_r = D.dice_probs(truth, probs, 1e-7, reduce, 0.7)
    loss, ws, td = K.dice_fwd(probs.to(dev), truth.to(dev), 1e-7, reduce)
    grad = K.dice_bwd(td, probs.shape, reduce, ws, torch.full((), 0.7, device=dev))
    grad1 = K.dice_bwd(td, probs.shape, reduce, ws, None)
    print("dice C=%d %s: loss %.8g (ref %.8g) grad %.3g" % (c, reduce, float(loss), float(loss_r), rel_err(grad, grad_r)))
    assert _close(loss, loss_r)
    assert rel_err(grad, grad_r) < 1e-4 and rel_err(grad1, grad_r / 0.7) < 1e-4
    loss_b, ws_b, _ = K.dice_fwd(probs.to(dev), truth.to(dev), 1e-7, reduce)
    assert torch.equal(loss_b, loss) and torch.equal(K.dice_bwd(td, probs.shape, reduce, ws_b, None), grad1)


@pytest.mark.parametrize("reduce", ["class", "sample"])
@pytest.mark.parametrize("activation", [True, False])
@pytest.mark.parametrize("c", [1, 3, 16])
def test_dice_loss_with_the_jaccard_signature(dev, c, activation, reduce):
    """autograd through the activation: C == 1 pairs [sigmoid, 1 - sigmoid] with ``true`` broadcast, C > 1 goes through a
    softmax (``activation``) or takes its input as probabilities"""
    from pointcloududa_amd.utils import loss as L
    rng = np.random.default_rng(31 * c + activation)
    n, h, w = 2, 1, 257
    x = _rand(rng, n, c, h, w, scale=2.0)
    if not activation and c > 1:
        x = torch.softmax(x, 1)
    true = _onehot(rng, n, c, h * w).view(n, c, h, w)
    loss_r, grad_r = D.dice_signature(true, x, 1e-7, activation, reduce)
    xd = x.to(dev).requires_grad_(True)
    loss = L.dice_loss(true.to(dev), xd, 1e-7, activation, reduce)
    loss.backward()
    print("dice_loss C=%d act=%d %s: loss %.8g (ref %.8g) grad %.3g" % (c, activation, reduce, float(loss.detach()), float(loss_r),
                                                                         rel_err(xd.grad, grad_r)))
    assert _close(loss, loss_r) and rel_err(xd.grad, grad_r) < 1e-4
    # fp32 truth holding the same zeros and ones: the other reader, the same arithmetic
    assert torch.equal(L.dice_loss(true.float().to(dev), xd.detach(), 1e-7, activation, reduce), loss.detach())


LABELS = [(2, c, 1, 257) for c in (2, 5, 16)] + [(1, 2, 513, 512)]


@pytest.mark.parametrize("dtype", [torch.uint8, torch.int64], ids=["u8", "i64"])
@pytest.mark.parametrize("n,c,h,w", LABELS, ids=["C2", "C5", "C16", "C2-513x512"])
def test_dice_loss_module_on_label_maps(dev, n, c, h, w, dtype):
    from pointcloududa_amd.utils import loss as L
    rng = np.random.default_rng(13 * c + h)
    logits = _rand(rng, n, c, h, w, scale=2.0)
    lab = torch.from_numpy(rng.integers(0, c, (n, h, w))).to(dtype)
    loss_r, grad_r, nbad = D.dice_labels(logits, lab, 1e-6, 0.7)
    assert nbad == 0
    m = L.DiceLoss()
    ld = logits.to(dev).requires_grad_(True)
    loss = m(ld, lab.to(dev))
    (loss * 0.7).backward()
    print("DiceLoss C=%d %s: loss %.8g (ref %.8g) grad %.3g" % (c, dtype, float(loss), float(loss_r), rel_err(ld.grad, grad_r)))
    assert _close(loss, loss_r) and rel_err(ld.grad, grad_r) < 1e-4
    assert int(m.bad_labels) == 0
    # the same value as the stand-alone form on the one-hot tensor this form never writes
    onehot = torch.nn.functional.one_hot(lab.long(), c).movedim(-1, 1).to(torch.uint8).contiguous()
    other = L.dice_loss(onehot.to(dev), logits.to(dev), 1e-6, True, "sample")
    assert _close(loss, other)
    # the same bits from a second run
    ld2 = logits.to(dev).requires_grad_(True)
    loss2 = L.DiceLoss()(ld2, lab.to(dev))
    (loss2 * 0.7).backward()
    assert torch.equal(loss2, loss) and torch.equal(ld2.grad, ld.grad)


@pytest.mark.parametrize("dtype", [torch.uint8, torch.int64], ids=["u8", "i64"])
def test_labels_outside_the_classes_are_counted_ignored_and_raised(dev, dtype):
    from pointcloududa_amd.utils import loss as L
    rng = np.random.default_rng(5)
    n, c, h, w = 2, 5, 3, 101
    logits = _rand(rng, n, c, h, w, scale=2.0)
    lab = torch.from_numpy(rng.integers(0, c, (n, h, w))).to(dtype)
    lab[0, 0, :7] = c                      # the first label past the classes
    lab[1, 2, 50:53] = 200
    if dtype == torch.int64:
        lab[1, 1, :5] = -1
        lab[0, 2, 100] = 2 ** 40 + 1       # (its low bits name a class: the whole value is read)
    loss_r, grad_r, nbad = D.dice_labels(logits, lab, 1e-6)
    assert nbad == (16 if dtype == torch.int64 else 10)
    m = L.DiceLoss()
    ld = logits.to(dev).requires_grad_(True)
    loss = m(ld, lab.to(dev))
    loss.backward()
    assert int(m.bad_labels) == nbad
    assert _close(loss, loss_r) and rel_err(ld.grad, grad_r) < 1e-4
    with pytest.raises(ValueError, match="outside"):
        L.DiceLoss(check=True)(logits.to(dev), lab.to(dev))
    assert float(L.DiceLoss(check=True)(logits.to(dev), lab.clamp(0, c - 1).to(dev))) > 0


def test_dice_loss_module_rejects_what_kornia_rejects(dev):
    from pointcloududa_amd.utils import loss as L
    m = L.DiceLoss()
    x, y = torch.zeros(2, 3, 4, 4, device=dev), torch.zeros(2, 4, 4, dtype=torch.int64, device=dev)
    with pytest.raises(ValueError):
        m(x[0], y)
    with pytest.raises(ValueError):
        m(x, y[:, :, :3])
    with pytest.raises(ValueError):
        m(x, y.cpu())
    with pytest.raises(TypeError):
        m(x, y.int())
    assert float(m(x, y)) > 0


@pytest.mark.parametrize("mode", ["sigmoid", "softmax"])
def test_the_jaccard_default_is_the_unchanged_path(dev, mode):
    from pointcloududa_amd import kernels as K
    from pointcloududa_amd.utils import loss as L
    logits, onehot, _ = _fused_inputs(4, 3, 300)
    ld, od = logits.to(dev), onehot.to(dev)
    out2, ws = K.seg_loss_fwd(ld, od, mode)
    one = torch.ones((), device=dev)
    grad = K.seg_loss_bwd(ld, od, mode, ws, one, one)
    for args in ((), ("jaccard",)):
        l = ld.clone().requires_grad_(True)
        a, b = L.seg_loss(l, od, mode, *args)
        assert torch.equal(a, out2[0]) and torch.equal(b, out2[1])
        (a + b).backward()
        assert torch.equal(l.grad, grad)
    l = ld.clone().requires_grad_(True)
    a, b = L.seg_loss(l, od, mode, "dice")
    assert _close(a, out2[0])                                  # the same main term, from the other kernel
    assert abs(float(b) - float(out2[1])) > 1e-3               # another overlap term


# ------------------------------------------------------------------------------------------ the callers
STEP_KW = dict(filters=4, in_channels=1, n_class=4, pointnet=True, fc_inch=9)


def _step(dev, dice):
    from oracle.synth import synth_batch
    from test_step_gpu import _build
    _, tr = _build(STEP_KW, 77, dev, dice=dice)
    batch = [torch.from_numpy(t).to(dev) for t in synth_batch(4, 1, 4, 128, seed=177)]
    out = tr.step(*batch, keep=True)
    return tr, batch, out


@pytest.fixture(scope="module")
def plain_step(dev):
    return _step(dev, "")


@pytest.mark.parametrize("dice", ["class", "sample"])
def test_train_step_with_the_dice_switch(dev, dice, plain_step):
    from pointcloududa_amd.train_step import AdversarialTrainer
    tr, batch, out = _step(dev, dice)
    o_s = tr.last["oS"]
    main_r, dice_r, _ = D.seg_loss_dice(o_s, batch[1], "sigmoid", dice, EPS[dice])
    print("step dice=%s: loss_dice %.8g (ref %.8g) loss_bce %.8g (ref %.8g)" % (
        dice, float(out["loss_dice"]), float(dice_r), float(out["loss_bce"]), float(main_r)))
    assert _close(out["loss_dice"], dice_r) and _close(out["loss_bce"], main_r)
    assert torch.equal(out["loss_jac"], out["loss_dice"])
    h = AdversarialTrainer.to_host(out, tr.cfg)
    assert np.isfinite(h["seg_loss"]) and abs(h["seg_loss"] - (h["loss_bce"] + h["loss_dice"])) < 1e-6
    # the supervised gradient changed with the loss: same weights, same batch, another overlap term
    tr0, _, out0 = plain_step
    assert torch.equal(tr0.last["oS"], o_s)
    assert set(out) - set(out0) == {"loss_dice"} and set(out0) - set(out) == set()
    assert not torch.equal(tr0.last["grad_seg"], tr.last["grad_seg"])


def test_train_step_without_the_switch_is_todays(dev, plain_step):
    from pointcloududa_amd import kernels as K
    tr0, batch, out0 = plain_step
    assert "loss_dice" not in out0
    assert set(out0) == {"loss_bce", "loss_jac", "ver_s_loss", "seg_dice", "ver_t_loss", "adv1", "adv2", "adv4", "d1_loss_src",
                         "d1_loss_tgt", "d2_loss_src", "d2_loss_tgt", "d4_loss_src", "d4_loss_tgt", "dis1_hit_src", "dis1_hit_tgt",
                         "dis2_hit_src", "dis2_hit_tgt", "dis4_hit_src", "dis4_hit_tgt"}
    out2, _ = K.seg_loss_fwd(tr0.last["oS"], batch[1], "sigmoid")
    assert torch.equal(out0["loss_bce"], out2[0]) and torch.equal(out0["loss_jac"], out2[1])


def test_train_epoch_reads_args_dice(dev):
    """``args.dice=True`` changes the supervised term of the epoch (the per-class Dice in the Jaccard term's place); the value
    is read from ``args`` at every epoch, the cached trainer included"""
    from oracle.synth import synth_batch
    from test_epoch_gpu import _gen, _nets
    import pointcloududa_amd.train_mscmrseg as TM
    batches = [synth_batch(4, 1, 4, 128, seed=3300)]
    res = {}
    for dice in (False, True):
        _, _, (gen, d1, d2, d4) = _nets(dev, STEP_KW, 3200)
        og = torch.optim.Adam(gen.parameters(), lr=1e-3, betas=(0.9, 0.99))
        mk = lambda m: torch.optim.SGD(m.parameters(), lr=2.5e-5, momentum=0.99, weight_decay=0.0005)
        o1, o2, o4 = mk(d1), mk(d2), mk(d4)
        TM.args = types.SimpleNamespace(d1=True, d2=True, d4=True, dr=0.01, wp=1.0, dice=dice)
        res[dice] = TM.train_epoch(gen, d2, d4, d1, og, o2, o4, o1, _gen(batches, "A"), _gen(batches, "B"))
        assert gen._pcuda_trainer[1].cfg.dice == ("class" if dice else "")
    assert np.isfinite(res[True]["seg_loss"]) and abs(res[True]["seg_loss"] - res[False]["seg_loss"]) > 1e-3
    assert set(res[True]) == set(res[False])
    # the cached trainer follows args from one epoch to the next
    TM.args.dice = False
    again = TM.train_epoch(gen, d2, d4, d1, og, o2, o4, o1, _gen(batches, "A"), _gen(batches, "B"))
    assert gen._pcuda_trainer[1].cfg.dice == "" and np.isfinite(again["seg_loss"])


@pytest.mark.parametrize("variant,dice", [("mscmrseg", "class"), ("mmwhs", "sample")])
def test_valid_batch_with_the_dice_switch(dev, variant, dice):
    from oracle.synth import synth_batch
    from pointcloududa_amd import validate as V
    from test_epoch_gpu import _nets
    ms = variant == "mscmrseg"
    cin, nc = (1, 4) if ms else (3, 5)
    _, _, (gen, _, _, _) = _nets(dev, dict(STEP_KW, in_channels=cin, n_class=nc), 3400)
    gen.eval()
    x, y, z = [torch.from_numpy(t).to(dev) for t in synth_batch(3, cin, nc, 128, seed=3401, gaussian=not ms)[:3]]
    with torch.no_grad():
        pred = gen(x)[0]
    r = V.valid_batch(gen, x, y, z, d4=False, variant=variant, dice=dice)
    main_r, dice_r, _ = D.seg_loss_dice(pred, y, "sigmoid" if ms else "softmax", dice, EPS[dice])
    print("valid_batch %s %s: loss %.8g (ref %.8g)" % (variant, dice, float(r["loss"]), float(main_r + dice_r)))
    assert _close(r["loss"], main_r + dice_r)
    r0 = V.valid_batch(gen, x, y, z, d4=False, variant=variant)
    assert abs(float(r0["loss"]) - float(r["loss"])) > 1e-3
