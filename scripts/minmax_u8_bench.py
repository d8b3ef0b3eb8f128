"""Device time per call of the fp32 -> uint8 -> fp32 joint of the MM-WHS heavy path (DESIGN.md section 6, f6b;
utils/augment.py ``rescale="minmax_u8"``, csrc/augment.hip), fp32 [16,256,256,3] (config 4's per-rank shape) and
[32,256,256,3], 5 classes, no crop:

  minmax                     the batch-global (min, max) pair, two launches
  quantize_u8                fp32 -> uint8 with that pair, into a tensor that exists (4 B read + 1 B written per element)
  assemble_dequant           the dequantising assemble on the quantised images, mmwhs_light parameters
  assemble_div255            pcuda_augment_assemble with AUG_DIV255 on the same uint8 data: the same kernel, another table
  light_fused_minmax         minmax + the fused "minmax" launch (what rescale="minmax" runs)
  light_two_step_minmax_u8   minmax + quantize_u8 + assemble_dequant: the same bits with the uint8 images written out

The last two document why "minmax" stays the default for recipes without uint8 stages (and why "minmax_u8" without a plan or
program takes the fused launch).  Every figure is device-event time with the host running ahead of the device
(scripts/augment_bench.py ``device_ms``).  The quantiser is reported as a share of the float4-copy rate on record
(profiles/resample_bench.json ``copy_bytes_per_s``) on its 5 bytes per element.

    python scripts/minmax_u8_bench.py [--iters 200] [--out profiles/minmax_u8_bench.json]"""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "scripts"))
import make_augment_golden as G  # noqa: E402
from augment_bench import device_ms  # noqa: E402
from oracle.synth import synth_batch  # noqa: E402
from pointcloududa_amd import _lib  # noqa: E402
from pointcloududa_amd import kernels as KK  # noqa: E402
from pointcloududa_amd.utils.augment import sample_params, upload_params  # noqa: E402

H, W, C, K = 256, 256, 3, 5


def copy_rate():
    with open(os.path.join(ROOT, "profiles", "resample_bench.json")) as f:
        rec = json.load(f)
    rec = rec[0] if isinstance(rec, list) else rec
    return float(rec["copy_bytes_per_s"])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--out", default=None, help="also write the result lines to this JSON file")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("minmax_u8_bench: needs a HIP device")
    dev = torch.device("cuda", 0)
    rate = copy_rate()
    results = []
    for b in (16, 32):
        x = np.concatenate([G.smooth_images(8, H, W, C, 7 + i) for i in range(b // 8)])
        lab = np.argmax(synth_batch(b, 1, K, H, seed=3)[1], axis=1).astype(np.int32)
        tx, tl = torch.from_numpy(x).to(dev), torch.from_numpy(lab).to(dev)
        up = upload_params(sample_params(b, "mmwhs_light", np.random.default_rng(1)), b, H, W, dev)
        mm = KK.minmax(tx)
        q = KK.quantize_u8(tx, mm)
        assert np.array_equal(q.cpu().numpy(), G.quantise(x)[0])
        fused = KK.augment_assemble(tx, tl, *up, K, 0, KK.AUG_MINMAX, mm)
        two = KK.augment_assemble_dequant(q, tl, *up, mm, K, 0)
        assert torch.equal(fused["images"], two["images"]) and torch.equal(fused["onehot"], two["onehot"])

        def two_step():
            m = KK.minmax(tx)
            return KK.augment_assemble_dequant(KK.quantize_u8(tx, m, out=q), tl, *up, m, K, 0)

        def fused_call():
            return KK.augment_assemble(tx, tl, *up, K, 0, KK.AUG_MINMAX, KK.minmax(tx))
        ms = {
            "minmax": device_ms(lambda: KK.minmax(tx), args.iters),
            "quantize_u8": device_ms(lambda: KK.quantize_u8(tx, mm, out=q), args.iters),
            "assemble_dequant": device_ms(lambda: KK.augment_assemble_dequant(q, tl, *up, mm, K, 0), args.iters),
            "assemble_div255": device_ms(lambda: KK.augment_assemble(q, tl, *up, K, 0, KK.AUG_DIV255), args.iters),
            "light_fused_minmax": device_ms(fused_call, args.iters),
            "light_two_step_minmax_u8": device_ms(two_step, args.iters),
        }
        n = tx.numel()
        q_rate = 5.0 * n / (ms["quantize_u8"] * 1e-3)
        r = {"shape": [b, H, W, C], "classes": K, "iters": args.iters, "build": _lib.csrc_hash(),
             "ms": {k: round(v, 5) for k, v in ms.items()},
             "quantize_u8_bytes_per_s": round(q_rate, -9), "copy_bytes_per_s": rate,
             "quantize_u8_fraction_of_copy_rate": round(q_rate / rate, 4),
             "minmax_bytes_per_s": round(4.0 * n / (ms["minmax"] * 1e-3), -9),
             "dequant_over_div255": round(ms["assemble_dequant"] / ms["assemble_div255"], 3),
             "two_step_over_fused": round(ms["light_two_step_minmax_u8"] / ms["light_fused_minmax"], 3)}
        results.append(r)
        print(json.dumps(r), flush=True)
    if args.out:
        with open(args.out, "w") as f:
            json.dump(results, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
