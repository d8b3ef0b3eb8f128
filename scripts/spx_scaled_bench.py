"""Device time per call of superpixels at a working size (utils/stylize.py ``max_size``, csrc/spx_scale.hip; DESIGN.md section 6,
f9c), B = 32, 256x256x3 uint8 (6.3 MB), one SUPERPIXELS slot per sample, 5 updates, p_replace 0.5, at n_segments = 20 and 200,
four slots in one process:

  * ``unscaled``: max_size = 0, min_size = 0 through pcuda_stylize (f9's slot: unchanged code, the yardstick)
  * ``connected``: max_size = 0, min_size = superpixel_min_size through pcuda_stylize_connect (f9b's slot, the other yardstick)
  * ``scaled``: max_size = 128, min_size = 0 through pcuda_stylize_scaled (the grid is that of the 128 x 128 working size)
  * ``scaled_connected``: max_size = 128, min_size = superpixel_min_size on the working size, through pcuda_stylize_scaled

and ``scaled_entry_unscaled_program``: the ``connected`` program through pcuda_stylize_scaled (what a batch that scales nothing
pays for the entry point's extra launches).  From one profiled call per scaled setting, the device time of each kernel.  Timed
with the host running ahead of the device (a spin kernel goes first), as scripts/spx_connect_bench.py.  The requirement
(recorded as ``scaled_below_unscaled``): the scaled slot takes less device time than the unscaled one at both segment counts.

    python scripts/spx_scaled_bench.py [--iters 50] [--out profiles/spx_scaled_bench.json]"""
import argparse
import json
import os
import re
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "scripts"))
import make_stylize_golden as G  # noqa: E402
from augment_bench import device_ms  # noqa: E402
from pointcloududa_amd import _lib  # noqa: E402
from pointcloududa_amd import kernels as KK  # noqa: E402
from pointcloududa_amd.utils import stylize as S  # noqa: E402

B, H, W, C = 32, 256, 256, 3
P_REPLACE = 0.5


def program(n_segments, connected, max_size):
    hs, ws = S.superpixel_working_size(H, W, max_size)
    gy, gx = S.superpixel_grid(n_segments, hs, ws)
    prog = S.StyleProgram.identity(B, 1)
    for i in range(B):
        prog.set_superpixels(i, 0, gy, gx, P_REPLACE, 1234567 + i, min_size=S.superpixel_min_size(gy, gx, hs, ws) if connected else 0,
                             max_size=max_size)
    return prog


def kernel_split(fn):
    """device microseconds per kernel name of one call, or None where the profiler is not available"""
    try:
        from torch.profiler import ProfilerActivity, profile
        with profile(activities=[ProfilerActivity.CUDA]) as p:
            fn()
            torch.cuda.synchronize()
        out = {}
        for e in p.key_averages():
            t = getattr(e, "device_time_total", None)
            if t is None:
                t = getattr(e, "cuda_time_total", 0.0)
            m = re.search(r"((?:spx_connect|spx_scale|stylize)_\w+_kernel)", e.key)
            if t and m:
                out[m.group(1)] = round(out.get(m.group(1), 0.0) + float(t), 1)
        return out or None
    except Exception as e:      # noqa: BLE001 (a measurement aid: the timings above do not depend on it)
        return {"error": repr(e)[:200]}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--out", default=None, help="also write the result to this JSON file")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("spx_scaled_bench: needs a HIP device")
    dev = torch.device("cuda", 0)
    x = np.concatenate([G.make_images("grey3", 16, H, W, C, 71), G.make_images("smooth", 8, H, W, C, 72),
                        G.make_images("random", 8, H, W, C, 73)])
    tx = torch.from_numpy(x).to(dev)
    out = torch.empty_like(tx)
    r = {"shape": [B, H, W, C], "iters": args.iters, "build": _lib.csrc_hash(), "copy_bytes": 2 * x.size, "p_replace": P_REPLACE,
         "max_size": S.SUPERPIXELS_MAX_SIZE, "working_size": list(S.superpixel_working_size(H, W, S.SUPERPIXELS_MAX_SIZE)),
         "inputs": "16 grey3, 8 smooth, 8 uniform noise (make_stylize_golden.make_images)",
         "torch_copy_ms": round(device_ms(lambda: out.copy_(tx), args.iters), 4)}
    for n in (20, 200):
        up = {(conn, m): S.upload_style_program(program(n, conn, m), B, H, W, C, dev)
              for conn in (False, True) for m in (0, S.SUPERPIXELS_MAX_SIZE)}
        m = S.SUPERPIXELS_MAX_SIZE
        d = {"grid_unscaled": list(S.superpixel_grid(n, H, W)), "grid_scaled": list(S.superpixel_grid(n, m, m)),
             "unscaled_ms": device_ms(lambda: KK.stylize(tx, *up[False, 0], out=out), args.iters),
             "connected_ms": device_ms(lambda: KK.stylize(tx, *up[True, 0], out=out, connect=True), args.iters),
             "scaled_ms": device_ms(lambda: KK.stylize_scaled(tx, *up[False, m], out=out), args.iters),
             "scaled_connected_ms": device_ms(lambda: KK.stylize_scaled(tx, *up[True, m], out=out), args.iters),
             "scaled_entry_unscaled_program_ms": device_ms(lambda: KK.stylize_scaled(tx, *up[True, 0], out=out), args.iters)}
        d = {k: (round(v, 4) if isinstance(v, float) else v) for k, v in d.items()}
        d["scaled_below_unscaled"] = bool(d["scaled_ms"] < d["unscaled_ms"])
        d["scaled_connected_below_connected"] = bool(d["scaled_connected_ms"] < d["connected_ms"])
        d["kernel_us_one_call_scaled"] = kernel_split(lambda: KK.stylize_scaled(tx, *up[False, m], out=out))
        d["kernel_us_one_call_scaled_connected"] = kernel_split(lambda: KK.stylize_scaled(tx, *up[True, m], out=out))
        r["n_segments_%d" % n] = d
    r["clock_ghz_under_load"] = round(KK.clock_ghz_under_load(dev), 3)
    print(json.dumps(r), flush=True)
    if args.out:
        with open(args.out, "w") as f:
            json.dump(r, f, indent=1)
            f.write("\n")
    if not all(r["n_segments_%d" % n]["scaled_below_unscaled"] for n in (20, 200)):
        raise SystemExit("spx_scaled_bench: the scaled slot is not below the unscaled one")


if __name__ == "__main__":
    main()
