"""Device time of the native-size evaluation of MS-CMRSeg (csrc/area_resize.hip) for one batch of a
patient's slices, logits fp32 [16,4,224,224] in a 256 canvas, to 480 x 480 and to 512 x 512 (the sizes of real LGE label files):

  fused    kernels.reconstruct_resize_argmax: one kernel, logits in, uint8 labels out
  unfused  the reference's order with every intermediate in memory: the zero canvas and the paste (torch), C calls of
           kernels.area_resize (one per class plane, as resize_volume is called), kernels.argmax_labels over the stacked planes

Both paths run behind the same warm-up and alternate in the same process (three rounds, the median is kept, all rounds are in the
file); the host runs ahead of the device (a spin kernel goes first), so the figures are device time.  The labels of the two paths
are compared bit for bit before anything is timed.

Bytes: what the task must move -- the logits read once, the labels written once -- over the device time gives the achieved
bytes/s, beside the fraction of the float4-copy rate that profiles/resample_bench.json records (6.29 TB/s).  The unfused chain's
own traffic (its passes added up) is recorded next to it.

    python scripts/area_resize_bench.py [--iters 50] [--out profiles/area_resize_bench.json]"""
import argparse
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "scripts"))
from augment_bench import device_ms  # noqa: E402
from pointcloududa_amd import _lib  # noqa: E402
from pointcloududa_amd import kernels as KK  # noqa: E402

N, C, SIDE, CROP, ORIGIN = 16, 4, 224, 112, 256
ROUNDS = 3


def unfused(logits, h, w):
    o = ORIGIN // 2
    canvas = torch.zeros((N, C, ORIGIN, ORIGIN), dtype=torch.float32, device=logits.device)
    canvas[:, :, o - CROP:o + CROP, o - CROP:o + CROP] = logits
    planes = torch.stack([KK.area_resize(canvas[:, k], h, w) for k in range(C)], dim=1)
    return KK.argmax_labels(planes)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--out", default=None, help="also write the result to this JSON file")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("area_resize_bench: needs a HIP device")
    dev = torch.device("cuda", 0)
    with open(os.path.join(ROOT, "profiles", "resample_bench.json")) as f:
        copy_rate = float(json.load(f)["copy_bytes_per_s"])
    torch.manual_seed(0)
    logits = torch.randn((N, C, SIDE, SIDE), dtype=torch.float32, device=dev) * 2.0 - 0.5
    cases = {}
    for side in (480, 512):
        equal = bool(torch.equal(KK.reconstruct_resize_argmax(logits, side, side, CROP, ORIGIN), unfused(logits, side, side)))
        runs = {"fused": lambda: KK.reconstruct_resize_argmax(logits, side, side, CROP, ORIGIN),
                "unfused": lambda: unfused(logits, side, side)}
        times = {k: [] for k in runs}
        for _ in range(ROUNDS):                                           # the paths alternate
            for k, fn in runs.items():
                times[k].append(device_ms(fn, args.iters))
        must = N * C * SIDE * SIDE * 4 + N * side * side                  # the logits once, the labels once
        planes = N * C * side * side * 4
        canvas = N * C * ORIGIN * ORIGIN * 4
        r = {"fused_equals_unfused": equal, "bytes_must_move": must,
             # the chain's passes: the canvas zeroed and pasted into, read by the resizes, the planes written, stacked (read and
             # written), read by argmax, the labels written
             "bytes_unfused_chain_moves": canvas + 2 * N * C * SIDE * SIDE * 4 + canvas + planes + 2 * planes + planes + N * side * side}
        for k, v in times.items():
            r[k + "_ms_rounds"] = [float("%.4g" % t) for t in v]
            r[k + "_ms"] = float("%.4g" % statistics.median(v))
        rate = must / (r["fused_ms"] * 1e-3)
        r["fused_bytes_per_s"] = float("%.4g" % rate)
        r["fused_fraction_of_copy_rate"] = float("%.4g" % (rate / copy_rate))
        r["unfused_over_fused"] = float("%.4g" % (r["unfused_ms"] / r["fused_ms"]))
        cases["%dx%d" % (side, side)] = r
    res = {"logits": [N, C, SIDE, SIDE], "crop": CROP, "origin": ORIGIN, "iters": args.iters, "rounds": ROUNDS, "build": _lib.csrc_hash(),
           "copy_bytes_per_s": copy_rate, "cases": cases, "clock_ghz_under_load": round(KK.clock_ghz_under_load(dev), 3),
           "host_threads": os.environ.get("OMP_NUM_THREADS")}
    print(json.dumps(res), flush=True)
    if args.out:
        with open(args.out, "w") as f:
            json.dump(res, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
