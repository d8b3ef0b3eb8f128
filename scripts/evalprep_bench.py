"""Device time of the test-volume reader (utils/volume.py, csrc/evalprep.hip) at the size of an MM-WHS
CT volume, 256 x 256 x 256, against the ATen chain a user of the same device would write today:

  ours    evaluate_mmwhs.read_volume's image half: pcuda_volume_slices -> fp32 [256,3,256,256], one kernel
  aten    vol.permute(2, 0, 1).flip(1, 2)[table].contiguous().float(), table = [[i - 1, i, (i + 1) % D]]: a flip copy, a gather
          copy of three times the volume, and (for int16) a cast pass

for an int16 and an fp32 volume, each in C order (the slice axis fastest in memory: the tile kernel over z) and in Fortran order
(what a NIfTI reader returns, the first axis fastest: the tile kernel over r), and the whole read_volume (image and a uint8 mask)
next to the chain for both.  Both paths run behind the same warm-up and alternate in the same process (three rounds, the median
is kept, all rounds are in the file); the host runs ahead of the device (a spin kernel goes first), so the figures are device
time.  The outputs of the two paths are compared bit for bit before anything is timed.

Bytes: what the task must move -- the volume read once, the fp32 stack written once -- is the same for both paths; over the
device time it gives the achieved bytes/s, beside the fraction of the float4-copy rate that profiles/resample_bench.json
records.  The ATen chain's own traffic (its passes added up) is recorded next to it.

    python scripts/evalprep_bench.py [--iters 50] [--out profiles/evalprep_bench.json]"""
import argparse
import json
import os
import statistics
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "scripts"))
from augment_bench import device_ms  # noqa: E402
from pointcloududa_amd import _lib  # noqa: E402
from pointcloududa_amd import evaluate_mmwhs as EW  # noqa: E402
from pointcloududa_amd import kernels as KK  # noqa: E402
from pointcloududa_amd.utils import volume as VOL  # noqa: E402

SIDE = 256
ROUNDS = 3


def aten_image(vol, table):
    return vol.permute(2, 0, 1).flip(1, 2)[table].contiguous().float()


def aten_mask(mask):
    return mask.permute(2, 0, 1).flip(1, 2).contiguous().to(torch.uint8)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--out", default=None, help="also write the result to this JSON file")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("evalprep_bench: needs a HIP device")
    dev = torch.device("cuda", 0)
    with open(os.path.join(ROOT, "profiles", "resample_bench.json")) as f:
        copy_rate = float(json.load(f)["copy_bytes_per_s"])
    n = SIDE ** 3
    rng = np.random.default_rng(0)
    table = torch.tensor([[(i - 1) % SIDE, i, (i + 1) % SIDE] for i in range(SIDE)], device=dev)
    mask_c = rng.integers(0, 5, (SIDE, SIDE, SIDE), dtype=np.uint8)
    cases = {}
    for name, dtype in (("int16", np.int16), ("fp32", np.float32)):
        host = rng.integers(-1000, 3000, (SIDE, SIDE, SIDE)).astype(dtype)
        for order in ("C", "F"):
            vol = VOL.as_device_volume(np.asfortranarray(host) if order == "F" else host)
            mask = VOL.as_device_volume(np.asfortranarray(mask_c) if order == "F" else mask_c)
            out = torch.empty((SIDE, 3, SIDE, SIDE), dtype=torch.float32, device=dev)
            view = vol.movedim(2, 0)
            equal = bool(torch.equal(KK.volume_slices(view, True, True, 3, out=out), aten_image(vol, table)))
            equal_mask = bool(torch.equal(EW.read_volume(vol, mask, check=False)[1], aten_mask(mask)))
            runs = {"ours_slices": lambda: KK.volume_slices(view, True, True, 3, out=out),
                    "aten_slices": lambda: aten_image(vol, table),
                    "ours_read_volume": lambda: EW.read_volume(vol, mask, check=False),
                    "aten_read_volume": lambda: (aten_image(vol, table), aten_mask(mask))}
            times = {k: [] for k in runs}
            for _ in range(ROUNDS):                                       # the paths alternate
                for k, fn in runs.items():
                    times[k].append(device_ms(fn, args.iters))
            es = vol.element_size()
            must = n * es + 12 * n                                        # the volume once, the stack once
            must_rv = must + n + n                                        # + the uint8 mask once, the labels once
            r = {"strides": list(vol.stride()), "equal_to_aten": equal, "labels_equal_to_aten": equal_mask,
                 "bytes_must_move_slices": must, "bytes_must_move_read_volume": must_rv,
                 # the chain's passes: the flip copy, the gather (three times the volume in and out), the cast (int16 only)
                 "bytes_aten_chain_moves_slices": 2 * n * es + 6 * n * es + (3 * n * es + 12 * n if es != 4 else 0)}
            for k, v in times.items():
                r[k + "_ms_rounds"] = [float("%.4g" % t) for t in v]
                r[k + "_ms"] = float("%.4g" % statistics.median(v))
            for k, nbytes in (("slices", must), ("read_volume", must_rv)):
                rate = nbytes / (r["ours_%s_ms" % k] * 1e-3)
                r["ours_%s_bytes_per_s" % k] = float("%.4g" % rate)
                r["ours_%s_fraction_of_copy_rate" % k] = float("%.4g" % (rate / copy_rate))
                r["aten_over_ours_%s" % k] = float("%.4g" % (r["aten_%s_ms" % k] / r["ours_%s_ms" % k]))
            cases["%s_%s" % (name, order)] = r
            del vol, mask, out, view
            torch.cuda.empty_cache()
    res = {"volume": [SIDE, SIDE, SIDE], "iters": args.iters, "rounds": ROUNDS, "build": _lib.csrc_hash(), "copy_bytes_per_s": copy_rate,
           "cases": cases, "clock_ghz_under_load": round(KK.clock_ghz_under_load(dev), 3), "host_threads": os.environ.get("OMP_NUM_THREADS")}
    print(json.dumps(res), flush=True)
    if args.out:
        with open(args.out, "w") as f:
            json.dump(res, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
