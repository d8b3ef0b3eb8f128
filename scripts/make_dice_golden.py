#!/usr/bin/env python3
"""Writes tests/golden/dice_loss.npz: small logits, one-hot truths, and the Dice losses and gradients of tests/dice_refs.py
in both activation modes and both reductions, in float64.

The Dice rule is this build's own (include/pcuda_hip.h), so there is no reference run to record.  Instead the fixture is
computed twice and independently -- torch autograd over the definition, and the closed-form gradient in plain numpy -- and
the script refuses to write unless the two agree to 1e-12.  The larger shapes it also checks, (1, 2, 262656) among them,
stay out of the fixture (a committed file is small).

    python scripts/make_dice_golden.py            # CPU only
"""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import dice_refs as D      # noqa: E402

EPS = {"class": 1e-7, "sample": 1e-6}           # what seg_loss uses for the two reductions
STORED = [(2, 3, 257), (3, 1, 1), (1, 2, 1031)]
CHECKED_ONLY = [(1, 2, 262656)]
AGREE = 1e-12


def make_case(n, c, hw, seed):
    rng = np.random.default_rng(seed)
    logits = rng.normal(0, 2.0, (n, c, hw)).astype(np.float32)
    if c == 1:
        onehot = rng.integers(0, 2, (n, 1, hw)).astype(np.uint8)
    else:
        onehot = np.moveaxis(np.eye(c, dtype=np.uint8)[rng.integers(0, c, (n, hw))], -1, 1).copy()
    return torch.from_numpy(logits), torch.from_numpy(onehot)


def both(logits, onehot, mode, reduce):
    """(loss, gradient) of the two restatements after checking that they agree"""
    la, ga = D.dice_autograd(logits, onehot, mode, reduce, EPS[reduce])
    lc, gc = D.dice_closed_form(logits, onehot, mode, reduce, EPS[reduce])
    dl = abs(float(la) - float(lc))
    dg = float(np.abs(ga.numpy() - gc).max())
    if not (dl <= AGREE and dg <= AGREE):
        raise SystemExit("the two restatements disagree at %s %s %s: loss %.3g gradient %.3g: nothing written"
                         % (tuple(logits.shape), mode, reduce, dl, dg))
    return float(la), ga.numpy(), max(dl, dg)


def main():
    out, worst = {"shapes": np.array(STORED, dtype=np.int64)}, 0.0
    for i, (n, c, hw) in enumerate(STORED + CHECKED_ONLY):
        logits, onehot = make_case(n, c, hw, 4100 + i)
        stored = i < len(STORED)
        if stored:
            out["c%d/logits" % i], out["c%d/onehot" % i] = logits.numpy(), onehot.numpy()
        for mode in ("sigmoid", "softmax"):
            for reduce in ("class", "sample"):
                loss, grad, d = both(logits, onehot, mode, reduce)
                worst = max(worst, d)
                if stored:
                    out["c%d/%s/%s/loss" % (i, mode, reduce)] = np.float64(loss)
                    out["c%d/%s/%s/grad" % (i, mode, reduce)] = grad
    out["eps_class"], out["eps_sample"] = np.float64(EPS["class"]), np.float64(EPS["sample"])
    path = os.path.join(ROOT, "tests", "golden", "dice_loss.npz")
    np.savez_compressed(path, **out)
    print("wrote %s (%d bytes); the two restatements agree to %.3g" % (path, os.path.getsize(path), worst))


if __name__ == "__main__":
    main()
