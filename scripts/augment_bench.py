"""Device time per call of the loader tail with and without the device-side light augmentation (utils/augment.py,
csrc/augment.hip), B = 32, 256x256x3, 5 classes, crop 0 and 224:

  (a) assemble_batch                                   the parent's pass (crop, HWC -> CHW, one-hot)
  (b) augment_batch, identity parameters, no rescale   the same result through the new kernel
  (c) augment_batch, mmwhs_light parameters + min-max  min-max reduction + warp + rescale + assembly
  (c_mask_fused / c_mask_split)  (c) plus the full-size sampler mask, written by the same launch / by a second launch
  (d) (c) with resample_verts                          plus the point-cloud sampler (one host synchronisation of its own)

(a), (b), (c) and the two mask variants are timed at the kernel wrappers with the parameters already on the device and the
host running ahead of the device; a_call / c_call / d are the public entry points as a loader calls them (parameters
composed on the host and uploaded per call), where the host's issue time shows.

Algorithmic bytes from the shapes: read 4C + 4 per gathered pixel, write 4C + K per output pixel, plus 1 per full-size pixel
for the sampler mask, plus 4C per pixel for the min-max pass.  Also the host time of the scipy restatement
(scripts/make_augment_golden.py) of (c) where scipy is importable.

    python scripts/augment_bench.py [--iters 200] [--out profiles/augment_bench.json]"""
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
import make_augment_golden as G  # noqa: E402
from oracle.synth import synth_batch  # noqa: E402
from pointcloududa_amd import _lib  # noqa: E402
from pointcloududa_amd import kernels as KK  # noqa: E402
from pointcloududa_amd.utils.augment import AugmentParams, augment_batch, sample_params, upload_params  # noqa: E402
from pointcloududa_amd.utils.batch import assemble_batch  # noqa: E402

B, H, W, C, K = 32, 256, 256, 3, 5


def device_ms(fn, iters, ahead=True):
    """device-event time per call over ``iters`` warmed calls.  ``ahead``: a 20 ms spin kernel goes first, so that the host
    has queued the calls before the device reaches the first event and the figure is the device's time, not the time the
    host needs to issue a call (the kernels here run for tens of microseconds)"""
    for _ in range(10):
        fn()
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    if ahead:
        torch.cuda._sleep(40_000_000)
    a.record()
    for _ in range(iters):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / iters


def scipy_ms(x, lab, params):
    """the host restatement of (c): quantise, warp every channel and the mask, de-quantise"""
    try:
        import scipy  # noqa: F401
    except ImportError:
        return None
    p = {k: getattr(params, k) for k in G.PARAM_KEYS}
    t0 = time.perf_counter()
    q, mn, mx = G.quantise(x)
    inv = G.compose_inverse(p, params.op_order, H, W)
    order, cval = G.effective(p)
    out = np.empty_like(q)
    for i in range(B):
        for ch in range(C):
            out[i, :, :, ch] = G.to_u8(G.warp_scipy(q[i, :, :, ch], inv[i], order[i], cval[i]))
        G.to_u8(G.warp_scipy(lab[i], inv[i], 0, 0))
    G.dequantise(out, mn, mx)
    return round(1e3 * (time.perf_counter() - t0), 1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--out", default=None, help="also write the result lines to this JSON file")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("augment_bench: needs a HIP device")
    dev = torch.device("cuda", 0)
    x = np.concatenate([G.smooth_images(8, H, W, C, 7 + i) for i in range(B // 8)])
    lab = np.argmax(synth_batch(B, 1, K, H, seed=3)[1], axis=1).astype(np.int64)
    tx, tl = torch.from_numpy(x).to(dev), torch.from_numpy(lab).to(dev)
    params = sample_params(B, "mmwhs_light", np.random.default_rng(1))
    ident = AugmentParams.identity(B)
    results = []
    for crop in (0, 224):
        oh = ow = crop if crop else H
        out_pix, full_pix = B * oh * ow, B * H * W
        base = out_pix * (4 * C + 4 + 4 * C + K)
        with_mask = base + full_pix * 4 * C + full_pix
        nbytes = {"a": base, "b": base, "c": base + full_pix * 4 * C, "c_mask_fused": with_mask, "c_mask_split": with_mask}
        up_i, up_p = upload_params(ident, B, H, W, dev), upload_params(params, B, H, W, dev)
        tl32 = tl.to(torch.int32)
        ms = {
            "a": device_ms(lambda: KK.assemble_batch(tx, tl32, K, crop), args.iters),
            "b": device_ms(lambda: KK.augment_assemble(tx, tl32, *up_i, K, crop, KK.AUG_NONE), args.iters),
            "c": device_ms(lambda: _rescaled(tx, tl32, up_p, crop, False, False), args.iters),
            "c_mask_fused": device_ms(lambda: _rescaled(tx, tl32, up_p, crop, True, True), args.iters),
            "c_mask_split": device_ms(lambda: _rescaled(tx, tl32, up_p, crop, True, False), args.iters),
            # the public entry points, parameters composed and uploaded per call, as a loader calls them; (d) synchronises
            "a_call": device_ms(lambda: assemble_batch(tx, tl, K, crop), args.iters, ahead=False),
            "c_call": device_ms(lambda: augment_batch(tx, tl, params, K, crop, rescale="minmax"), args.iters, ahead=False),
            "d": device_ms(lambda: augment_batch(tx, tl, params, K, crop, rescale="minmax", resample_verts=True),
                           max(20, args.iters // 10), ahead=False),
        }
        r = {"shape": [B, H, W, C], "classes": K, "crop": crop, "iters": args.iters, "build": _lib.csrc_hash(),
             "ms": {k: round(v, 4) for k, v in ms.items()},
             "gbps": {k: round(nbytes[k] / (ms[k] * 1e6), 1) for k in nbytes},
             "c_over_a": round(ms["c"] / ms["a"], 3), "b_over_a": round(ms["b"] / ms["a"], 3),
             "predicted_c_over_a": round((12 * C + K + 5) / (8 * C + K + 4), 3),
             "scipy_c_ms": scipy_ms(x, lab, params) if crop == 0 else None}
        results.append(r)
        print(json.dumps(r), flush=True)
    if args.out:
        with open(args.out, "w") as f:
            json.dump(results, f, indent=1)
            f.write("\n")


def _rescaled(tx, lab, up, crop, mask, fused):
    """(c): min-max reduction + warp + rescale + assembly on parameters that are already on the device; ``mask``: plus the
    full-size sampler mask (without the sampler itself), from the same launch (``fused``) or from a second one"""
    mm = KK.minmax(tx)
    out = KK.augment_assemble(tx, lab, *up, K, crop, KK.AUG_MINMAX, mm, want_full_mask=mask and fused)
    if mask and not fused:
        out["full_mask"] = KK.augment_assemble(tx, lab, *up, K, crop, KK.AUG_MINMAX, mm, want_images=False, want_onehot=False,
                                               want_full_mask=True)["full_mask"]
    return out


if __name__ == "__main__":
    main()
