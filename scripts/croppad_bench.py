"""Device time per call of the device-side CropAndPad with numpy's pad modes (utils/croppad.py, csrc/croppad.hip) at B = 32,
256x256x3, every sample live with sides (13, 20, -9, 26) (inside the recipe's -5 % .. +10 %), once per mode:

  (a) kernels.crop_pad with the output preallocated (the workspace comes from torch's caching allocator), with and without
      int32 masks, the host running ahead of the device (a spin kernel goes first); next to it, on the same inputs,
      kernels.geometric with ONE crop-and-pad slot (f8's kernel, unchanged by f14; it knows the five index modes only, so the
      other five are measured in its constant mode) and a copy of the image tensor by torch (the byte bound)
  (b) crop_pad_aug as a loader calls it (validation, pinned upload of the program), host not ahead

The call is three kernels (the line statistics, the pad-row statistics and ramp flags, the sampling pass); samples whose mode
needs no statistic leave the first two at once.  Their split comes from a kernel trace of one mode in a run of its own
(rocprofv3 --kernel-trace --stats -- python scripts/croppad_bench.py --iters 20 --modes MEDIAN).

    python scripts/croppad_bench.py [--iters 200] [--modes MEAN,MEDIAN] [--out profiles/croppad_bench.json]"""
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
from pointcloududa_amd.utils import croppad as Cp  # noqa: E402
from pointcloududa_amd.utils import geometric as Geo  # noqa: E402

B, H, W, C = 32, 256, 256, 3
SIDES = (13, 20, -9, 26)
GEO_MODE = {Cp.MODE_CONSTANT: Geo.MODE_CONSTANT, Cp.MODE_EDGE: Geo.MODE_EDGE, Cp.MODE_REFLECT: Geo.MODE_REFLECT,
            Cp.MODE_SYMMETRIC: Geo.MODE_SYMMETRIC, Cp.MODE_WRAP: Geo.MODE_WRAP}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--modes", default=",".join(Cp.MODE_NAMES), help="comma-separated mode names (a kernel trace of one mode)")
    ap.add_argument("--out", default=None, help="also write the result to this JSON file")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("croppad_bench: needs a HIP device")
    dev = torch.device("cuda", 0)
    rng = np.random.default_rng(3)
    x = torch.from_numpy(rng.integers(0, 256, (B, H, W, C), dtype=np.uint8)).to(dev)
    lab = torch.from_numpy(rng.integers(0, 5, (B, H, W)).astype(np.int32)).to(dev)
    out, lab_out = torch.empty_like(x), torch.empty_like(lab)
    res = {}
    for mode, name in enumerate(Cp.MODE_NAMES):
        if name not in args.modes.split(","):
            continue
        prog = Cp.CropPadProgram.identity(B)
        geo = Geo.GeoProgram.identity(B, 1)
        for i in range(B):
            prog.set_crop_and_pad(i, *SIDES, mode, 128)
            geo.set_crop_and_pad(i, 0, H, W, *SIDES, GEO_MODE.get(mode, Geo.MODE_CONSTANT), 128)
        up = Cp.upload_crop_pad_program(prog, B, H, W, dev)
        gup = Geo.upload_geo_program(geo, B, H, W, dev)
        r = {"a_crop_pad_ms": device_ms(lambda: KK.crop_pad(x, None, *up, out=out), args.iters),
             "a_crop_pad_masks_ms": device_ms(lambda: KK.crop_pad(x, lab, *up, out=out, labels_out=lab_out), args.iters),
             "a_geometric_one_slot_ms": device_ms(lambda: KK.geometric(x, None, *gup, out=out), args.iters),
             "geometric_mode": Geo.MODE_NAMES[GEO_MODE.get(mode, Geo.MODE_CONSTANT)],
             "b_crop_pad_aug_call_ms": device_ms(lambda: Cp.crop_pad_aug(x, None, prog), args.iters, ahead=False)}
        res[name] = {k: (round(v, 4) if isinstance(v, float) else v) for k, v in r.items()}
    r = {"shape": [B, H, W, C], "sides_top_right_bottom_left": list(SIDES), "cval": 128, "iters": args.iters,
         "bytes_image": int(x.numel()), "workspace_bytes": int(_lib.lib().pcuda_crop_pad_workspace_size(B, H, W, C)),
         "a_torch_copy_u8_ms": round(device_ms(lambda: out.copy_(x), args.iters), 4), "build": _lib.csrc_hash(), "modes": res,
         "clock_ghz_under_load": round(KK.clock_ghz_under_load(dev), 3)}
    print(json.dumps(r), flush=True)
    if args.out:
        with open(args.out, "w") as f:
            json.dump(r, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
