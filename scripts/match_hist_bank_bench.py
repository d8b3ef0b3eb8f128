"""Device time per call of histogram matching against a reference bank (utils/histmatch.py HistReferenceBank,
csrc/histmatch_bank.hip) at B = 32, 256x256x3, fp32 and uint8:

  bank_of_32   match_histograms' kernels (kernels.match_hist_bank, output preallocated), sample i against reference i
  bank_of_1    the same against a bank of one (every sample reads the same reference plane)
  build_32 / build_1   kernels.hist_bank_build into preallocated storage (what HistReferenceBank.rebuild runs)
  fixed        kernels.match_hist of the fixed-reference path (csrc/histmatch.hip) on the same images, in the same run
  torch_copy   a copy of the image tensor by torch

Every figure is the median of ROUNDS rounds of ``--iters`` calls timed with device events, the host running ahead of the
device (scripts/augment_bench.py device_ms); the rounds themselves are kept.  Beside each time: the bytes the call must move
at least (the images read and written; for a build the references read and the bank written) per second, as a fraction of
the 6.29 TB/s a float4 copy reaches on this part (profiles/resample_bench.json).  Nothing is asserted on: this records.

    python scripts/match_hist_bank_bench.py [--iters 100] [--out profiles/match_hist_bank_bench.json]"""
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
import make_match_hist_golden as G  # noqa: E402
from augment_bench import device_ms  # noqa: E402
from pointcloududa_amd import _lib  # noqa: E402
from pointcloududa_amd import kernels as KK  # noqa: E402
from pointcloududa_amd.utils.histmatch import HistReference  # noqa: E402

B, SIDE, C = 32, 256, 3
ROUNDS = 5
COPY_BYTES_PER_S = 6.29e12


def inputs(kind, seed):
    if kind == "f32":
        return G.normal_f32((B, SIDE, SIDE, C), seed, 100.0, 300.0), G.normal_f32((B, SIDE, SIDE, C), seed + 1, 0.0, 1.0)
    return G.smooth_u8((B, SIDE, SIDE, C), seed), G.smooth_u8((B, SIDE, SIDE, C), seed + 1)


def timed(fn, iters, nbytes):
    rounds = [device_ms(fn, iters) for _ in range(ROUNDS)]
    ms = statistics.median(rounds)
    return {"ms": round(ms, 4), "rounds_ms": [round(v, 4) for v in rounds],
            "fraction_of_copy_rate": float("%.4g" % (nbytes / (ms * 1e-3) / COPY_BYTES_PER_S))}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=100)
    ap.add_argument("--out", default=None, help="also write the result to this JSON file")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("match_hist_bank_bench: needs a HIP device")
    dev = torch.device("cuda", 0)
    res = {}
    for kind in ("f32", "u8"):
        img, refs = inputs(kind, 11 + (kind == "u8"))
        tx, tr = torch.from_numpy(img).to(dev), torch.from_numpy(refs).to(dev)
        out = torch.empty_like(tx)
        moved = 2 * img.nbytes
        r = {"image_bytes": int(img.nbytes), "planes": B * C, "values_per_plane": SIDE * SIDE}
        for size in (B, 1):
            sub = tr[:size].contiguous()
            bank, ws, flag = KK.hist_bank_build(sub)
            idx = (torch.arange(B, dtype=torch.int32, device=dev) if size == B else torch.zeros(B, dtype=torch.int32, device=dev))
            r["bank_of_%d_bytes" % size] = int(bank.numel())
            r["build_%d" % size] = timed(lambda: KK.hist_bank_build(sub, bank, ws, flag), args.iters, sub.numel() * sub.element_size()
                                         + bank.numel())
            r["bank_of_%d" % size] = timed(lambda: KK.match_hist_bank(tx, bank, sub.shape, idx, out=out), args.iters, moved)
            want = np.concatenate([G.match_unique(img[i:i + 1], refs[int(idx[i])] + refs.dtype.type(0)) for i in (0, B - 1)])
            r["bank_of_%d_equal_to_numpy" % size] = bool(np.array_equal(out[[0, B - 1]].cpu().numpy(), want))
        ref = HistReference(refs[0], dev)
        r["fixed"] = timed(lambda: KK.match_hist(tx, ref.values, ref.quantiles, ref.lengths, out=out), args.iters, moved)
        r["torch_copy"] = timed(lambda: out.copy_(tx), args.iters, moved)
        res["%s_%dx%dx%d" % (kind, SIDE, SIDE, C)] = r
    r = {"batch": B, "iters": args.iters, "rounds": ROUNDS, "build": _lib.csrc_hash(), "copy_bytes_per_s": COPY_BYTES_PER_S,
         "cases": res, "clock_ghz_under_load": round(KK.clock_ghz_under_load(dev), 3)}
    print(json.dumps(r), flush=True)
    if args.out:
        with open(args.out, "w") as f:
            json.dump(r, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
