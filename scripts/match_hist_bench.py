"""Device time per call of the device-side histogram matching (utils/histmatch.py, csrc/histmatch.hip), B = 16 (the
reference's batch), C = 3, at 256x256 (the MM-WHS slices) and 512x512, fp32 and uint8:

  (a) kernels.match_hist with the output preallocated (the workspace comes from torch's caching allocator), next to a copy of
      the same tensor by torch (the byte bound), with the host running ahead of the device (a spin kernel goes first)
  (b) match_histograms as a loader calls it, host not ahead (where the host's issue time shows)
  (c) the plain-numpy restatement (np.unique / np.interp, scripts/make_match_hist_golden.py) on this machine's host CPU

The fp32 call is two kernels (the per-plane sort, then the per-value lookup); their split comes from a kernel trace of this
script in a run of its own (rocprofv3 --kernel-trace --stats -- python scripts/match_hist_bench.py --iters 20 --no-host).

    python scripts/match_hist_bench.py [--iters 200] [--no-host] [--out profiles/match_hist_bench.json]"""
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
import make_match_hist_golden as G  # noqa: E402
from augment_bench import device_ms  # noqa: E402
from pointcloududa_amd import _lib  # noqa: E402
from pointcloududa_amd import kernels as KK  # noqa: E402
from pointcloududa_amd.utils.histmatch import HistReference, match_histograms  # noqa: E402

B, C = 16, 3


def inputs(kind, side, seed):
    if kind == "f32":
        return G.normal_f32((B, side, side, C), seed, 100.0, 300.0), G.normal_f32((side, side, C), seed + 1, 0.0, 1.0)
    return G.smooth_u8((B, side, side, C), seed), G.smooth_u8((1, side, side, C), seed + 1)[0]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--no-host", action="store_true", help="skip the numpy restatement (c)")
    ap.add_argument("--out", default=None, help="also write the result to this JSON file")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("match_hist_bench: needs a HIP device")
    dev = torch.device("cuda", 0)
    res = {}
    for kind in ("f32", "u8"):
        for side in (256, 512):
            img, refimg = inputs(kind, side, 7 * side + (kind == "u8"))
            tx, ref = torch.from_numpy(img).to(dev), HistReference(refimg, dev)
            out = torch.empty_like(tx)
            r = {"bytes": int(img.nbytes), "planes": B * C, "values_per_plane": side * side,
                 "workspace_bytes": int(_lib.lib().pcuda_match_hist_workspace_size(B, side, side, C, int(kind == "u8"))),
                 "a_kernels_ms": device_ms(lambda: KK.match_hist(tx, ref.values, ref.quantiles, ref.lengths, out=out), args.iters),
                 "a_torch_copy_ms": device_ms(lambda: out.copy_(tx), args.iters),
                 "b_call_ms": device_ms(lambda: match_histograms(tx, ref), args.iters, ahead=False)}
            if not args.no_host:
                t0 = time.perf_counter()
                want = G.match_unique(img, refimg)
                r["c_numpy_ms"] = 1e3 * (time.perf_counter() - t0)
                r["equal_to_numpy"] = bool(np.array_equal(out.cpu().numpy(), want))
            res["%s_%dx%d" % (kind, side, side)] = {k: (round(v, 4) if isinstance(v, float) else v) for k, v in r.items()}
    r = {"batch": B, "channels": C, "iters": args.iters, "build": _lib.csrc_hash(), "cases": res,
         "clock_ghz_under_load": round(KK.clock_ghz_under_load(dev), 3), "host_threads": os.environ.get("OMP_NUM_THREADS")}
    print(json.dumps(r), flush=True)
    if args.out:
        with open(args.out, "w") as f:
            json.dump(r, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
