"""Device time per call of the Dice losses (utils/loss.py, csrc/dice_loss.hip) next to the Jaccard path they stand beside, at
the two shapes the train steps run: [32,4,256,256] in sigmoid mode (MS-CMRSeg) and [16,5,256,256] in softmax mode (MM-WHS).

  (a) forward + backward of the fused seg_loss (kernels.seg_loss_fwd / _bwd) and of its two Dice forms
      (kernels.seg_loss_ov_fwd / _bwd, "dice" per class and "dice_sample" per sample), seeds given as the train step gives them
  (b) DiceLoss (logits + int64 label map, autograd forward + backward) against the equivalent ATen chain
      (softmax, one_hot, two products and sums, the ratio's mean, autograd backward)
  (c) dice_loss on given probabilities (kernels.dice_fwd / _bwd, both reductions) against jaccard_loss (kernels.jaccard_fwd / _bwd)

Every figure is measured --repeats times (device events around --iters calls, a spin kernel first so that the host is ahead);
the JSON holds the median and the spread (max - min) of each.  The Jaccard figures of (a) and (c) are the yardstick: the
per-class Dice form moves the same bytes (5 per element forward, 9 backward) and should lie within their spread.

    python scripts/dice_loss_bench.py [--iters 100] [--repeats 5] [--out profiles/dice_loss_bench.json]"""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "scripts"))
from augment_bench import device_ms  # noqa: E402
from pointcloududa_amd import _lib  # noqa: E402
from pointcloududa_amd import kernels as KK  # noqa: E402
from pointcloududa_amd.utils import loss as L  # noqa: E402

SHAPES = (("sigmoid", 32, 4, 256, 256), ("softmax", 16, 5, 256, 256))


def measure(fn, iters, repeats):
    v = sorted(device_ms(fn, iters) for _ in range(repeats))
    return {"ms": round(v[len(v) // 2], 5), "spread_ms": round(v[-1] - v[0], 5)}


def aten_dice(logits, labels, eps=1e-6):
    p = torch.softmax(logits, 1)
    y = torch.nn.functional.one_hot(labels, logits.shape[1]).movedim(-1, 1).to(p.dtype)
    inter, card = (p * y).sum((1, 2, 3)), (p + y).sum((1, 2, 3))
    return (1.0 - 2.0 * inter / (card + eps)).mean()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=100)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--out", default=None, help="also write the result to this JSON file")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("dice_loss_bench: needs a HIP device")
    dev = torch.device("cuda", 0)
    one = torch.ones((), device=dev)
    res = {}
    for mode, n, c, h, w in SHAPES:
        rng = np.random.default_rng(n + c)
        logits = torch.from_numpy(rng.normal(0, 2.0, (n, c, h, w)).astype(np.float32)).to(dev)
        lab = torch.from_numpy(rng.integers(0, c, (n, h, w))).to(dev)
        onehot = torch.nn.functional.one_hot(lab, c).movedim(-1, 1).to(torch.uint8).contiguous()
        probs = torch.sigmoid(logits) if mode == "sigmoid" else torch.softmax(logits, 1)
        m = lambda fn: measure(fn, args.iters, args.repeats)

        def fused_jaccard():
            _, ws = KK.seg_loss_fwd(logits, onehot, mode)
            KK.seg_loss_bwd(logits, onehot, mode, ws, one, one)

        def fused(overlap, eps):
            def run():
                _, ws = KK.seg_loss_ov_fwd(logits, onehot, mode, overlap, eps)
                KK.seg_loss_ov_bwd(logits, onehot, mode, overlap, ws, one, one)
            return run

        def on_probs_jaccard():
            _, ws, t = KK.jaccard_fwd(probs, onehot, 1e-7)
            KK.jaccard_bwd(t, probs.shape, 1e-7, ws, one)

        def on_probs(reduce):
            def run():
                _, ws, t = KK.dice_fwd(probs, onehot, 1e-7, reduce)
                KK.dice_bwd(t, probs.shape, reduce, ws, one)
            return run

        module = L.DiceLoss()

        def dice_module():
            l = logits.detach().requires_grad_(True)
            module(l, lab).backward()

        def dice_aten():
            l = logits.detach().requires_grad_(True)
            aten_dice(l, lab).backward()

        r = {"shape": [n, c, h, w],
             "a_seg_loss_jaccard": m(fused_jaccard), "a_seg_loss_dice": m(fused("dice", 1e-7)),
             "a_seg_loss_dice_sample": m(fused("dice_sample", 1e-6)),
             "a_seg_loss_jaccard_again": m(fused_jaccard),
             "c_jaccard_on_probs": m(on_probs_jaccard), "c_dice_on_probs_class": m(on_probs("class")),
             "c_dice_on_probs_sample": m(on_probs("sample"))}
        # (DiceLoss is a softmax loss at either shape: the mode only names the fused runs)
        r["b_dice_module"], r["b_dice_aten_chain"] = m(dice_module), m(dice_aten)
        res[mode] = r
    out = {"iters": args.iters, "repeats": args.repeats, "build": _lib.csrc_hash(), "figures": "median ms per forward + backward; spread_ms = max - min over the repeats",
           "shapes": res, "clock_ghz_under_load": round(KK.clock_ghz_under_load(dev), 3)}
    print(json.dumps(out), flush=True)
    if args.out:
        with open(args.out, "w") as f:
            json.dump(out, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
