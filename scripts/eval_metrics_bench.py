"""Device time per call of the evaluation kernels: kernels.surface_metrics (3 classes: dice, hd and asd both ways) and
kernels.largest_components on 20x256x256 and 32x256x256 label volumes (random blobs, scripts/make_eval_golden.py), and
the scipy restatement's time for the same metrics where scipy is importable.

    python scripts/eval_metrics_bench.py [--iters 50]        # one JSON line per shape"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "scripts"))
import make_eval_golden as G  # noqa: E402
from pointcloududa_amd import kernels as K  # noqa: E402


def device_ms(fn, iters):
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(iters):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / iters


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=50)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("eval_metrics_bench: needs a HIP device")
    dev = torch.device("cuda", 0)
    for z in (20, 32):
        gt = G.blobs((z, 256, 256), 41, [1, 2, 3], n=24)
        pred = G.blobs((z, 256, 256), 41, [1, 2, 3], n=24, shift=3)
        tp, tg = torch.from_numpy(pred.astype(np.uint8)).to(dev), torch.from_numpy(gt.astype(np.uint8)).to(dev)
        r = {"shape": [z, 256, 256],
             "surface_metrics_ms": round(device_ms(lambda: K.surface_metrics(tp, tg, [1, 2, 3]), args.iters), 4),
             "largest_components_ms": round(device_ms(lambda: K.largest_components(tp), args.iters), 4)}
        try:
            import scipy  # noqa: F401
            t0 = time.perf_counter()
            G.surface(pred, gt, [1, 2, 3])
            r["scipy_surface_ms"] = round(1e3 * (time.perf_counter() - t0), 1)
        except ImportError:
            r["scipy_surface_ms"] = None
        print(json.dumps(r), flush=True)


if __name__ == "__main__":
    main()
