"""Device time per call of the evaluation kernels: kernels.surface_metrics (3 classes: dice, hd and asd both ways),
kernels.surface_metrics_ext (+ hd95, assd), both at unit spacing and at (5.0, 1.2, 1.2) and taking turns in one process,
and kernels.largest_components, on 20x256x256 and 32x256x256 label volumes (random blobs, scripts/make_eval_golden.py);
and the scipy restatement's time for the same metrics where scipy is importable.

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


SPACING = (5.0, 1.2, 1.2)


def alternating_ms(fns, iters, rounds=3):
    """median over ``rounds`` of device_ms for each of ``fns``, the functions taking turns (one process, one warm-up)"""
    runs = [[] for _ in fns]
    for _ in range(rounds):
        for r, fn in zip(runs, fns):
            r.append(device_ms(fn, iters))
    return [round(float(np.median(r)), 4) for r in runs]


def host_hd95_assd_ms(pred, gt, classes, spacing):
    """the host path the extended call replaces: scipy's distance transform, np.percentile and the means, per class"""
    t0 = time.perf_counter()
    for c in classes:
        ab, ba = G.sd(pred == c, gt == c, spacing), G.sd(gt == c, pred == c, spacing)
        np.percentile(np.hstack((ab, ba)), 95)
        np.mean((ab.mean(), ba.mean()))
    return round(1e3 * (time.perf_counter() - t0), 1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=50)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("eval_metrics_bench: needs a HIP device")
    dev = torch.device("cuda", 0)
    cls = [1, 2, 3]
    for z in (20, 32):
        gt = G.blobs((z, 256, 256), 41, cls, n=24)
        pred = G.blobs((z, 256, 256), 41, cls, n=24, shift=3)
        tp, tg = torch.from_numpy(pred.astype(np.uint8)).to(dev), torch.from_numpy(gt.astype(np.uint8)).to(dev)
        plain, ext, plain_sp, ext_sp = alternating_ms(
            [lambda: K.surface_metrics(tp, tg, cls), lambda: K.surface_metrics_ext(tp, tg, cls),
             lambda: K.surface_metrics(tp, tg, cls, SPACING), lambda: K.surface_metrics_ext(tp, tg, cls, SPACING)], args.iters)
        r = {"shape": [z, 256, 256],
             "surface_metrics_ms": plain, "surface_metrics_ext_ms": ext,
             "surface_metrics_spacing_ms": plain_sp, "surface_metrics_ext_spacing_ms": ext_sp,
             "border_voxels": K.surface_metrics_ext(tp, tg, cls)[:, 10:].sum(1).tolist(),
             "largest_components_ms": round(device_ms(lambda: K.largest_components(tp), args.iters), 4)}
        try:
            import scipy  # noqa: F401
            t0 = time.perf_counter()
            G.surface(pred, gt, cls)
            r["scipy_surface_ms"] = round(1e3 * (time.perf_counter() - t0), 1)
            r["scipy_hd95_assd_ms"] = host_hd95_assd_ms(pred, gt, cls, None)
            r["scipy_hd95_assd_spacing_ms"] = host_hd95_assd_ms(pred, gt, cls, SPACING)
        except ImportError:
            r["scipy_surface_ms"] = r["scipy_hd95_assd_ms"] = r["scipy_hd95_assd_spacing_ms"] = None
        print(json.dumps(r), flush=True)


if __name__ == "__main__":
    main()
