"""Device time per call of the connected superpixels (utils/stylize.py ``min_size``, csrc/spx_connect.hip; DESIGN.md section 6,
f9b), B = 32, 256x256x3 uint8 (6.3 MB), one SUPERPIXELS slot per sample, 5 updates, at n_segments = 20 and 200:

  * ``connected``: pcuda_stylize_connect with min_size = superpixel_min_size on every sample
  * ``unconnected``: the same program with min_size = 0 through pcuda_stylize (f9's slot) in the same run
  * ``connected_entry_unconnected_program``: the min_size = 0 program through pcuda_stylize_connect (eight launches that leave
    at once: what a mixed batch pays for its unconnected samples)
  * ``torch_copy``: a uint8 copy of the batch (the byte bound)

and, from one profiled call per setting, the device time of each kernel of the pass (which phase dominates).  Timed with the
host running ahead of the device (a spin kernel goes first), as scripts/stylize_bench.py.  ``--bench-parent`` / ``--bench-this``
take files with bench.py's default line measured on the parent commit and on this tree (same box, alternating) and record
them next to the figures: the training step does not call these kernels, so its line must not move.

    python scripts/spx_connect_bench.py [--iters 50] [--out profiles/spx_connect_bench.json]
                                        [--bench-parent a.json b.json --bench-this c.json d.json]"""
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


def program(n_segments, connected):
    gy, gx = S.superpixel_grid(n_segments, H, W)
    prog = S.StyleProgram.identity(B, 1)
    for i in range(B):
        prog.set_superpixels(i, 0, gy, gx, 0.7, 1234567 + i, min_size=S.superpixel_min_size(gy, gx, H, W) if connected else 0)
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
            m = re.search(r"((?:spx_connect|stylize)_\w+_kernel)", e.key)
            if t and m:
                out[m.group(1)] = round(out.get(m.group(1), 0.0) + float(t), 1)
        return out or None
    except Exception as e:      # noqa: BLE001 (a measurement aid: the timings above do not depend on it)
        return {"error": repr(e)[:200]}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--out", default=None, help="also write the result to this JSON file")
    ap.add_argument("--bench-parent", nargs="*", default=[], help="files holding bench.py's JSON line, taken on the parent commit")
    ap.add_argument("--bench-this", nargs="*", default=[], help="the same on this tree, same box, alternating with the parent's")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("spx_connect_bench: needs a HIP device")
    dev = torch.device("cuda", 0)
    x = np.concatenate([G.make_images("grey3", 16, H, W, C, 71), G.make_images("smooth", 8, H, W, C, 72),
                        G.make_images("random", 8, H, W, C, 73)])
    tx = torch.from_numpy(x).to(dev)
    out = torch.empty_like(tx)
    r = {"shape": [B, H, W, C], "iters": args.iters, "build": _lib.csrc_hash(), "copy_bytes": 2 * x.size,
         "inputs": "16 grey3, 8 smooth, 8 uniform noise (make_stylize_golden.make_images)",
         "torch_copy_ms": round(device_ms(lambda: out.copy_(tx), args.iters), 4)}
    for n in (20, 200):
        on = S.upload_style_program(program(n, True), B, H, W, C, dev)
        off = S.upload_style_program(program(n, False), B, H, W, C, dev)
        d = {"grid": list(S.superpixel_grid(n, H, W)), "min_size": S.superpixel_min_size(*S.superpixel_grid(n, H, W), H, W),
             "connected_ms": device_ms(lambda: KK.stylize(tx, *on, out=out, connect=True), args.iters),
             "unconnected_ms": device_ms(lambda: KK.stylize(tx, *off, out=out), args.iters),
             "connected_entry_unconnected_program_ms": device_ms(lambda: KK.stylize(tx, *off, out=out, connect=True), args.iters)}
        d = {k: (round(v, 4) if isinstance(v, float) else v) for k, v in d.items()}
        d["pass_ms"] = round(d["connected_ms"] - d["unconnected_ms"], 4)
        d["kernel_us_one_call"] = kernel_split(lambda: KK.stylize(tx, *on, out=out, connect=True))
        r["n_segments_%d" % n] = d
    r["clock_ghz_under_load"] = round(KK.clock_ghz_under_load(dev), 3)
    if args.bench_parent or args.bench_this:      # the training step does not call these kernels: its line must not move
        line = lambda f: {k: v for k, v in json.loads(open(f).read().strip().splitlines()[-1]).items()
                          if k in ("value", "unit", "ms_per_step", "steps", "warmup", "launches_per_step")}
        r["bench_py_default_line"] = {"cmd": "python bench.py --gpus 1 --steps 20 --warmup 5",
                                      "parent": [line(f) for f in args.bench_parent], "this": [line(f) for f in args.bench_this]}
    print(json.dumps(r), flush=True)
    if args.out:
        with open(args.out, "w") as f:
            json.dump(r, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
