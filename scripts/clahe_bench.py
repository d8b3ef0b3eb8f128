"""Device time per call of the device-side slice preparation (utils/preprocess.py, csrc/preprocess.hip) at the reference's
224x224 slices, CLAHE with clip limit 2.0 on a 4x4 grid: one volume of 16 slices and a batch of 256 slices, and the whole
chain from a raw 256x256 int16 volume (rescale -> resize -> crop -> CLAHE -> fp32 [N,3,224,224]):

  (a) kernels.clahe / kernels.rescale_resize_crop_u8 with the output preallocated (the workspace comes from torch's caching
      allocator), next to a copy of the same tensor by torch (the byte bound), with the host running ahead of the device (a
      spin kernel goes first)
  (b) clahe / prepare_mscmrseg_slices as a loader calls them, host not ahead (where the host's issue time shows)
  (c) the vectorised numpy restatement (scripts/make_preprocess_golden.py) on this machine's host CPU

The CLAHE call is two kernels (the per-tile LUTs, then the blend); their split comes from a kernel trace of this script in a
run of its own (rocprofv3 --kernel-trace --stats -- python scripts/clahe_bench.py --iters 20 --no-host).

    python scripts/clahe_bench.py [--iters 200] [--no-host] [--out profiles/clahe_bench.json]"""
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
import make_preprocess_golden as G  # noqa: E402
from augment_bench import device_ms  # noqa: E402
from pointcloududa_amd import _lib  # noqa: E402
from pointcloududa_amd import kernels as KK  # noqa: E402
from pointcloududa_amd.utils.preprocess import clahe, prepare_mscmrseg_slices  # noqa: E402

SIDE, RAW = 224, 256


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--no-host", action="store_true", help="skip the numpy restatement (c)")
    ap.add_argument("--out", default=None, help="also write the result to this JSON file")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("clahe_bench: needs a HIP device")
    dev = torch.device("cuda", 0)
    res = {}
    for n in (16, 256):
        img = G.slices_u8((n, SIDE, SIDE), 7 + n)
        raw = (G.slices_u8((n, RAW, RAW), 70 + n).astype(np.int16) * 9 - 200)
        tx, tr = torch.from_numpy(img).to(dev), torch.from_numpy(raw).to(dev)
        out8, outf, outr = torch.empty_like(tx), torch.empty((n, 3, SIDE, SIDE), dtype=torch.float32, device=dev), torch.empty_like(tx)
        r = {"slices": n, "bytes_u8": int(img.nbytes), "bytes_f32x3": int(outf.numel() * 4),
             "workspace_bytes": int(_lib.lib().pcuda_clahe_workspace_size(n, 4, 4)),
             "a_clahe_u8_ms": device_ms(lambda: KK.clahe(tx, 2.0, 4, 4, False, out=out8), args.iters),
             "a_clahe_f32x3_ms": device_ms(lambda: KK.clahe(tx, 2.0, 4, 4, True, out=outf), args.iters),
             "a_rescale_resize_crop_ms": device_ms(lambda: KK.rescale_resize_crop_u8(tr, RAW, RAW, SIDE, out=outr), args.iters),
             "a_torch_copy_u8_ms": device_ms(lambda: out8.copy_(tx), args.iters),
             "a_torch_fill_f32x3_ms": device_ms(lambda: outf.fill_(0.5), args.iters),
             "b_clahe_call_ms": device_ms(lambda: clahe(tx), args.iters, ahead=False),
             "b_prepare_call_ms": device_ms(lambda: prepare_mscmrseg_slices(tr), args.iters, ahead=False)}
        KK.clahe(tx, 2.0, 4, 4, False, out=out8)
        if not args.no_host:
            t0 = time.perf_counter()
            want = G.clahe_numpy(img, 2.0, (4, 4))
            r["c_numpy_clahe_ms"] = 1e3 * (time.perf_counter() - t0)
            r["equal_to_numpy"] = bool(np.array_equal(out8.cpu().numpy(), want))
            t0 = time.perf_counter()
            want = G.to_float3(G.clahe_numpy(G.rescale_numpy(raw, RAW, RAW, SIDE), 2.0, (4, 4)))
            r["c_numpy_prepare_ms"] = 1e3 * (time.perf_counter() - t0)
            r["prepare_equal_to_numpy"] = bool(np.array_equal(prepare_mscmrseg_slices(tr).cpu().numpy(), want))
        res["%d_slices_%dx%d" % (n, SIDE, SIDE)] = {k: (round(v, 4) if isinstance(v, float) else v) for k, v in r.items()}
    r = {"clip_limit": 2.0, "grid": [4, 4], "iters": args.iters, "build": _lib.csrc_hash(), "cases": res,
         "clock_ghz_under_load": round(KK.clock_ghz_under_load(dev), 3), "host_threads": os.environ.get("OMP_NUM_THREADS")}
    print(json.dumps(r), flush=True)
    if args.out:
        with open(args.out, "w") as f:
            json.dump(r, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
