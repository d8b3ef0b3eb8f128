"""Pins every output bit of the loss entry points (csrc/losses.hip, csrc/dice_loss.hip) in tests/golden/loss_pin.json;
tests/test_loss_pin_gpu.py compares a build to it.

Run it on the build whose behaviour is to be kept (the PARENT of a refactor), never on the commit under test:

    python scripts/make_loss_pin_golden.py [--out tests/golden/loss_pin.json]        # needs the MI355X

It calls only the public functions of pointcloududa_amd.kernels, so the same file runs on either side of a refactor.  One
record per case: the case key, the ``launch_count()`` delta of the forward and of every backward call, the sha256 of the raw
bytes of every output tensor (scalars, gradients, maps, the bad-label counter) and of the inputs (a difference there is the
host's, not a kernel's).  Beside the records: ``torch.version.hip`` and the version line of hipcc.

Inputs: ``np.random.default_rng`` with a seed derived from the case's shape, normal(0, 2) logits, and, where hw >= 8, four
logits of +40 and four of -40 (the BCE log clamp, the softmax at its ends).  The kernels sum in a fixed order and use no
floating-point atomics, so the hashes repeat bit for bit."""
from __future__ import annotations

import math
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from pin_common import ROOT, K, _counted, _seed, _sha, recorder_main, toolchain, unique_cases  # noqa: E402,F401

OUT = os.path.join(ROOT, "tests", "golden", "loss_pin.json")

MODES = ("sigmoid", "softmax")
# fused forms: (name, eps); "jaccard" is seg_loss_fwd / _bwd, the others seg_loss_ov_fwd / _bwd
FUSED = (("jaccard", None), ("dice", 1e-7), ("dice_sample", 1e-6))
SEG_C = (1, 4, 5, 8)
# one pixel; a ragged block; three samples of more than a block; past the forward's 1024-block budget; past the backward's
# 4096 blocks; more samples than either budget
SEG_SHAPES = ((1, 1), (2, 257), (3, 300), (1, 513 * 512), (1, 1025 * 1024), (4100, 3))
PROB_SHAPES = ((2, 1, 257), (2, 16, 257), (1, 3, 257 * 256))
PROB_OPS = ("jaccard", "dice_class", "dice_sample")
ENT_SHAPES = ((2, 1, 257), (2, 2, 257), (2, 16, 257))
# the shapes scripts/dice_loss_bench.py times
PRODUCTION = (("sigmoid", 32, 4, 256 * 256), ("softmax", 16, 5, 256 * 256))


def _logits(rng, n, c, hw):
    x = rng.normal(0, 2.0, (n, c, hw)).astype(np.float32)
    if hw >= 8:
        x[0, 0, :4] = 40.0
        x[0, c - 1, 4:8] = -40.0
    return torch.from_numpy(x)


def _onehot(rng, n, c, hw):
    if c == 1:
        return torch.from_numpy(rng.integers(0, 2, (n, 1, hw)).astype(np.uint8))
    lab = rng.integers(0, c, (n, hw))
    return torch.from_numpy(np.moveaxis(np.eye(c, dtype=np.uint8)[lab], -1, 1).copy())


def _scalar(dev, v):
    return None if v is None else torch.full((), v, dtype=torch.float32, device=dev)


class _Inputs:
    """(logits, one-hot) of a shape, drawn once and kept on the device while consecutive cases share it"""

    def __init__(self, dev):
        self.dev, self.key, self.val = dev, None, None

    def get(self, n, c, hw):
        if self.key != (n, c, hw):
            rng = np.random.default_rng(_seed("seg", n, c, hw))
            logits, onehot = _logits(rng, n, c, hw), _onehot(rng, n, c, hw)
            self.key, self.val = (n, c, hw), (logits.to(self.dev), onehot.to(self.dev), {"logits": _sha(logits), "onehot": _sha(onehot)})
        return self.val


def _fused_record(key, form, eps, mode, ld, od, ins, g_main, g_ov):
    launches = {}
    if form == "jaccard":
        out2, ws = _counted(launches, "fwd", lambda: K.seg_loss_fwd(ld, od, mode))
        grad = _counted(launches, "bwd", lambda: K.seg_loss_bwd(ld, od, mode, ws, g_main, g_ov))
    else:
        out2, ws = _counted(launches, "fwd", lambda: K.seg_loss_ov_fwd(ld, od, mode, form, eps))
        grad = _counted(launches, "bwd", lambda: K.seg_loss_ov_bwd(ld, od, mode, form, ws, g_main, g_ov))
    return {"case": key, "launches": launches, "in": ins, "hash": {"out2": _sha(out2), "grad": _sha(grad)}}


def fused_cases(dev):
    inputs = _Inputs(dev)
    for c in SEG_C:
        for n, hw in SEG_SHAPES:
            ld, od, ins = inputs.get(n, c, hw)
            for form, eps in FUSED:
                for mode in MODES:
                    yield _fused_record("seg/%s/%s/C%d/%dx%d/g1-0.7" % (form, mode, c, n, hw), form, eps, mode, ld, od, ins,
                                        _scalar(dev, 1.0), _scalar(dev, 0.7))
    ld, od, ins = inputs.get(2, 4, 257)
    for form, eps in FUSED:
        for mode in MODES:
            yield _fused_record("seg/%s/%s/C4/2x257/gNone" % (form, mode), form, eps, mode, ld, od, ins, None, None)


def production_cases(dev):
    inputs = _Inputs(dev)
    for mode, n, c, hw in PRODUCTION:
        ld, od, ins = inputs.get(n, c, hw)
        for form, eps in FUSED:
            yield _fused_record("production/%s/%s/C%d/%dx%d/g1-1" % (form, mode, c, n, hw), form, eps, mode, ld, od, ins,
                                _scalar(dev, 1.0), _scalar(dev, 1.0))


def prob_cases(dev):
    for n, c, hw in PROB_SHAPES:
        for u8 in (True, False):
            rng = np.random.default_rng(_seed("probs", n, c, hw, u8))
            u = rng.random((n, c, hw), dtype=np.float32) + np.float32(0.05)
            probs = torch.from_numpy(u / u.sum(axis=1, keepdims=True)) if c > 1 else torch.from_numpy(u / np.float32(1.05))
            truth = _onehot(rng, n, c, hw) if u8 else torch.from_numpy(rng.random((n, c, hw), dtype=np.float32))
            ins = {"probs": _sha(probs), "truth": _sha(truth)}
            pd, td = probs.to(dev), truth.to(dev)
            for op in PROB_OPS:
                for gout in (None, 0.7):
                    launches = {}
                    g = _scalar(dev, gout)
                    if op == "jaccard":
                        loss, ws, t = _counted(launches, "fwd", lambda: K.jaccard_fwd(pd, td, 1e-7))
                        grad = _counted(launches, "bwd", lambda: K.jaccard_bwd(t, pd.shape, 1e-7, ws, g))
                    else:
                        red = op[len("dice_"):]
                        loss, ws, t = _counted(launches, "fwd", lambda: K.dice_fwd(pd, td, 1e-7, red))
                        grad = _counted(launches, "bwd", lambda: K.dice_bwd(t, pd.shape, red, ws, g))
                    yield {"case": "probs/%s/%dx%dx%d/%s/g%s" % (op, n, c, hw, "u8" if u8 else "f32", gout), "launches": launches,
                           "in": ins, "hash": {"loss": _sha(loss), "grad": _sha(grad)}}


def label_cases(dev):
    cases = [(2, 5, 257, "u8", False), (2, 5, 257, "i64", False), (2, 16, 257, "u8", False), (2, 16, 257, "i64", False),
             (2, 5, 257, "i64", True), (1, 2, 513 * 512, "u8", False)]
    for n, c, hw, kind, bad3 in cases:
        rng = np.random.default_rng(_seed("labels", n, c, hw))
        logits = _logits(rng, n, c, hw)
        lab = rng.integers(0, c, (n, hw))
        if bad3:      # below, just past and far past [0, c): no class, counted
            lab[0, 3], lab[0, 100], lab[n - 1, 7] = -1, c, 1000
        labels = torch.from_numpy(lab.astype(np.uint8 if kind == "u8" else np.int64))
        ld, labd = logits.to(dev), labels.to(dev)
        launches = {}
        loss, ws, lread, bad = _counted(launches, "fwd", lambda: K.dice_labels_fwd(ld, labd, 1e-6))
        grad = _counted(launches, "bwd", lambda: K.dice_labels_bwd(ld, lread, ws, _scalar(dev, 0.7)))
        yield {"case": "labels/%dx%dx%d/%s%s" % (n, c, hw, kind, "/bad3" if bad3 else ""), "launches": launches,
               "in": {"logits": _sha(logits), "labels": _sha(labels)},
               "hash": {"loss": _sha(loss), "bad": _sha(bad), "grad": _sha(grad)}}


def _norm(c, on):
    """1 / log C as train_mmwhs.py normalises (C = 1, where that is undefined: another multiplier that is not 1)"""
    return (1.0 / math.log(c) if c > 1 else 0.75) if on else 1.0


def entropy_cases(dev):
    for n, c, hw, norms in [s + ((False, True),) for s in ENT_SHAPES] + [(1, 2, 1025 * 1024, (True,))]:
        rng = np.random.default_rng(_seed("entropy", n, c, hw))
        logits = _logits(rng, n, c, hw)
        w1, w2, pre = (torch.from_numpy(rng.normal(0, 1.0, (n, c, hw)).astype(np.float32)) for _ in range(3))
        ins = {"logits": _sha(logits), "dent": _sha(w1), "dprob": _sha(w2), "pre": _sha(pre)}
        ld, w1d, w2d = logits.to(dev), w1.to(dev), w2.to(dev)
        dmd = _scalar(dev, 0.3 * n * hw)
        for mode in MODES:
            for on in norms:
                norm = _norm(c, on)
                launches = {}
                ent, prob = _counted(launches, "fwd", lambda: K.entropy_fwd(ld, mode, norm, want_prob=True))
                ent_only, _ = _counted(launches, "fwd_noprob", lambda: K.entropy_fwd(ld, mode, norm))
                h = {"ent": _sha(ent), "prob": _sha(prob), "ent_noprob": _sha(ent_only)}
                h["bwd_dent"] = _sha(_counted(launches, "bwd_dent", lambda: K.entropy_bwd(ld, mode, norm, dent=w1d)))
                h["bwd_dprob"] = _sha(_counted(launches, "bwd_dprob", lambda: K.entropy_bwd(ld, mode, norm, dprob=w2d)))
                h["bwd_dmean"] = _sha(_counted(launches, "bwd_dmean", lambda: K.entropy_bwd(ld, mode, norm, dmean=dmd)))
                h["bwd_all"] = _sha(_counted(launches, "bwd_all",
                                             lambda: K.entropy_bwd(ld, mode, norm, dent=w1d, dprob=w2d, dmean=dmd)))
                acc = pre.to(dev)
                _counted(launches, "bwd_acc", lambda: K.entropy_bwd(ld, mode, norm, dent=w1d, out=acc, accumulate=True))
                h["bwd_acc"] = _sha(acc)
                yield {"case": "entropy/%s/%dx%dx%d/norm%d" % (mode, n, c, hw, int(on)), "launches": launches, "in": ins, "hash": h}


def record(dev):
    """the records of every case, in a fixed order, of the library pointcloududa_amd._lib loads"""
    out = []
    for cases in (fused_cases, prob_cases, label_cases, entropy_cases, production_cases):
        out += list(cases(dev))
    torch.cuda.synchronize(dev)
    return unique_cases(out)


def main(argv):
    recorder_main("make_loss_pin_golden", argv, OUT,
                  "output hashes and launch counts of the loss entry points on the parent of the overlap-loss refactor "
                  "(scripts/make_loss_pin_golden.py)", record)


if __name__ == "__main__":
    main(sys.argv[1:])
