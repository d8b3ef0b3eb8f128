"""Device time per call of the device-side spacing resample (utils/resample.py, csrc/resample.hip) at the reference's sizes: a
raw 256x256 int16 volume of 16 and of 256 slices, zoomed to 267x267 (1.25 mm -> 1.2 mm) and cropped to 224x224:

  image chain   pcuda_zoom_standardize: table, zoom + partial sums, the final reduce, the map -> fp32 [N,3,224,224]
  label chain   pcuda_zoom_labels: table, the scan of the codes, the fused zoom / argmax -> uint8 [N,224,224]
  zoom alone    pcuda_zoom_linear_crop -> int16 [N,224,224]

  (a) the kernels.* wrappers with the output preallocated, the host running ahead of the device (a spin kernel goes first), next
      to torch copies of the same byte counts
  (b) the utils.resample calls as a loader makes them, host not ahead (where the host's issue time shows)

Bytes: what each chain must move -- the source rows the crop window reads (the whole input for the label chain's scan), the
result, and for the image chain the zoomed int16 values written once and read once -- over the device time gives the achieved
bytes/s; beside it the fraction of the 6.29 TB/s a float4 copy reaches on this part (MI355X_MICROARCH: HBM3E, measured).

    python scripts/resample_bench.py [--iters 200] [--out profiles/resample_bench.json]"""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "scripts"))
import make_resample_golden as G  # noqa: E402
from augment_bench import device_ms  # noqa: E402
from pointcloududa_amd import _lib  # noqa: E402
from pointcloududa_amd import kernels as KK  # noqa: E402
from pointcloududa_amd.utils import resample as R  # noqa: E402

RAW, ZOOMED, SIDE = 256, 267, 224
COPY_BYTES_PER_S = 6.29e12


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--out", default=None, help="also write the result to this JSON file")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("resample_bench: needs a HIP device")
    dev = torch.device("cuda", 0)
    factors = R.spacing_zoom_factors((RAW, RAW), (1.25, 1.25))
    assert R.zoom_output_shape((RAW, RAW), factors) == (ZOOMED, ZOOMED)
    # the source rows / columns the crop window touches
    iy, _, _ = G.axis_terms(RAW, ZOOMED)
    y0, x0, oh, ow = G.crop_window(ZOOMED, ZOOMED, SIDE)
    span = int(iy[y0 + oh - 1] + 1 - iy[y0] + 1)
    res = {}
    for n in (16, 256):
        raw = np.tile(G.smooth_volume((2, RAW, RAW), np.int16, 5), (n // 2, 1, 1))
        lab = np.tile(G.discs((0, 200, 500, 600), np.int16, 2), (n // 2, 11, 10))[:, :RAW, :RAW]
        tr, tl = torch.from_numpy(raw).to(dev), torch.from_numpy(np.ascontiguousarray(lab)).to(dev)
        outf = torch.empty((n, 3, SIDE, SIDE), dtype=torch.float32, device=dev)
        outz = torch.empty((n, SIDE, SIDE), dtype=torch.int16, device=dev)
        outl = torch.empty((n, SIDE, SIDE), dtype=torch.uint8, device=dev)
        stats = torch.empty(2, dtype=torch.float64, device=dev)
        px = n * SIDE * SIDE
        bytes_image = n * span * span * 2 + px * (2 + 2) + px * 12
        bytes_zoom = n * span * span * 2 + px * 2
        bytes_labels = n * RAW * RAW * 2 + n * span * span * 2 + px
        r = {"slices": n, "source_span": span,
             "a_image_chain_ms": device_ms(lambda: KK.zoom_standardize(tr, (ZOOMED, ZOOMED), SIDE, 3, out=outf, stats=stats), args.iters),
             "a_label_chain_ms": device_ms(lambda: KK.zoom_labels(tl, (ZOOMED, ZOOMED), 4, R.MSCMRSEG_REMAP, SIDE, out=outl), args.iters),
             "a_zoom_alone_ms": device_ms(lambda: KK.zoom_linear_crop(tr, (ZOOMED, ZOOMED), SIDE, out=outz), args.iters),
             "a_torch_copy_i16_input_ms": device_ms(lambda: tr.clone(), args.iters),
             "a_torch_fill_f32x3_ms": device_ms(lambda: outf.fill_(0.5), args.iters),
             "b_prepare_npy_call_ms": device_ms(lambda: R.prepare_mscmrseg_npy(tr, (1.25, 1.25)), args.iters, ahead=False),
             "b_prepare_npy_labels_call_ms": device_ms(lambda: R.prepare_mscmrseg_npy_labels(tl, (1.25, 1.25), check=False), args.iters, ahead=False),
             "bytes_image_chain": bytes_image, "bytes_label_chain": bytes_labels, "bytes_zoom_alone": bytes_zoom}
        for key, nbytes in (("image_chain", bytes_image), ("label_chain", bytes_labels), ("zoom_alone", bytes_zoom)):
            rate = nbytes / (r["a_%s_ms" % key] * 1e-3)
            r["%s_us" % key] = 1e3 * r["a_%s_ms" % key]
            r["%s_bytes_per_s" % key] = rate
            r["%s_fraction_of_copy_rate" % key] = rate / COPY_BYTES_PER_S
        # the results the timed calls left behind, against the restatement (one pair of slices; the volume repeats them)
        r["zoom_equal_to_rule"] = bool(np.array_equal(outz[:2].cpu().numpy(), G.zoom_rule(raw[:2], ZOOMED, ZOOMED, SIDE)))
        r["labels_equal_to_rule"] = bool(np.array_equal(outl[:2].cpu().numpy(), G.label_rule(lab[:2], ZOOMED, ZOOMED, 4, G.REMAP, SIDE)[0]))
        res["%d_slices" % n] = {k: (float("%.4g" % v) if isinstance(v, float) else v) for k, v in r.items()}
    r = {"raw": [RAW, RAW], "zoomed": [ZOOMED, ZOOMED], "crop": SIDE, "iters": args.iters, "build": _lib.csrc_hash(),
         "copy_bytes_per_s": COPY_BYTES_PER_S, "cases": res,
         "clock_ghz_under_load": round(KK.clock_ghz_under_load(dev), 3), "host_threads": os.environ.get("OMP_NUM_THREADS")}
    print(json.dumps(r), flush=True)
    if args.out:
        with open(args.out, "w") as f:
            json.dump(r, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
