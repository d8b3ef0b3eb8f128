"""Device time per call of Fourier domain adaptation against a bank (utils/fourier.py FourierBank / fourier_adapt,
csrc/fourier.hip) at B = 32, 256x256x3 and 224x224x1, fp32 and uint8, radius 2, 12 and 25:

  build        kernels.fourier_bank_build into preallocated storage (what FourierBank.rebuild runs), 32 references
  adapt        kernels.fourier_adapt, output preallocated, sample i against reference i
  aten_f64     the equivalent ATen chain on the device in float64, the arithmetic of the kernels: torch.fft.fft2 of the batch,
               abs / angle, the block of amplitudes replaced from a precomputed |T|, torch.polar, ifft2, real, the store's
               rounding (the targets' fft2 + abs is timed apart as aten_f64_build)
  aten_f32     the same chain in float32 / complex64 (what a user would write first; NOT the same result)
  torch_copy   a copy of the image tensor by torch

Every figure is the median of ROUNDS rounds of ``--iters`` calls timed with device events, the host running ahead of the
device (scripts/augment_bench.py device_ms); the rounds themselves are kept.  Beside each time of ours: the bytes the task must
move -- adapt: the source read twice and the output written once; build: the references read once -- per second, as a
fraction of the 6.29 TB/s a float4 copy reaches on this part (profiles/resample_bench.json), and ``ms_at_copy_rate``, the
time those bytes take at that rate.  ``max_abs_diff_aten_f64`` is the largest difference between our output and the float64
chain's (fp32 stores: one rounding apart at the most; uint8: pixels that differ).  If torch.fft does not work on the box
the aten entries hold the error text instead.  Nothing is asserted on: this records.

    python scripts/fourier_adapt_bench.py [--iters 50] [--out profiles/fourier_adapt_bench.json]"""
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
from pointcloududa_amd import kernels as KK  # noqa: E402

B = 32
SHAPES = ((256, 256, 3), (224, 224, 1))
RADII = (2, 12, 25)
ROUNDS = 5
COPY_BYTES_PER_S = 6.29e12


def timed(fn, iters, nbytes=None):
    rounds = [device_ms(fn, iters) for _ in range(ROUNDS)]
    ms = statistics.median(rounds)
    r = {"ms": round(ms, 4), "rounds_ms": [round(v, 4) for v in rounds]}
    if nbytes is not None:
        r["bytes"] = int(nbytes)
        r["ms_at_copy_rate"] = round(nbytes / COPY_BYTES_PER_S * 1e3, 4)
        r["fraction_of_copy_rate"] = float("%.4g" % (nbytes / (ms * 1e-3) / COPY_BYTES_PER_S))
    return r


def aten_chain(x, tamp, iy, ix, ctype):
    """``x`` [B,H,W,C] (fp32 or uint8) against precomputed block amplitudes ``tamp`` [B,2b+1,2b+1,C] -> the images' dtype"""
    rtype = torch.float64 if ctype == torch.complex128 else torch.float32
    S = torch.fft.fft2(x.to(rtype), dim=(1, 2))
    amp, ph = S.abs(), S.angle()
    amp[:, iy[:, None], ix[None, :]] = tamp
    v = torch.fft.ifft2(torch.polar(amp, ph), dim=(1, 2)).real
    if x.dtype == torch.uint8:
        return torch.round(v).clamp_(0, 255).to(torch.uint8)
    return v.to(torch.float32)


def aten_amplitudes(t, iy, ix, ctype):
    rtype = torch.float64 if ctype == torch.complex128 else torch.float32
    return torch.fft.fft2(t.to(rtype), dim=(1, 2)).abs()[:, iy[:, None], ix[None, :]].contiguous()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--out", default=None, help="also write the result to this JSON file")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("fourier_adapt_bench: needs a HIP device")
    dev = torch.device("cuda", 0)
    res = {}
    for h, w, c in SHAPES:
        for kind in ("f32", "u8"):
            rng = np.random.default_rng(7 + h + (kind == "u8"))
            img = rng.integers(0, 256, (B, h, w, c), dtype=np.uint8)
            refs = rng.integers(0, 256, (B, h, w, c), dtype=np.uint8)
            if kind == "f32":
                img, refs = img.astype(np.float32), refs.astype(np.float32)
            tx, tr = torch.from_numpy(img).to(dev), torch.from_numpy(refs).to(dev)
            out = torch.empty_like(tx)
            idx = torch.arange(B, dtype=torch.int32, device=dev)
            case = {"image_bytes": int(img.nbytes), "planes": B * c, "torch_copy": timed(lambda: out.copy_(tx), args.iters, 2 * img.nbytes)}
            for radius in RADII:
                bank, ws = KK.fourier_bank_storage(B, h, w, c, radius, dev)
                r = {"bank_bytes": int(bank.numel()), "build_workspace_bytes": int(ws.numel()),
                     "adapt_workspace_bytes": int(_lib.lib().pcuda_fourier_adapt_workspace_size(B, h, w, c, radius))}
                r["build"] = timed(lambda: KK.fourier_bank_build(tr, radius, bank, ws), args.iters, img.nbytes)
                r["adapt"] = timed(lambda: KK.fourier_adapt(tx, bank, B, radius, idx, out=out), args.iters, 3 * img.nbytes)
                ours = out.clone()
                iy = torch.from_numpy(np.arange(-radius, radius + 1) % h).to(dev)
                ix = torch.from_numpy(np.arange(-radius, radius + 1) % w).to(dev)
                for name, ctype in (("aten_f64", torch.complex128), ("aten_f32", torch.complex64)):
                    try:
                        tamp = aten_amplitudes(tr, iy, ix, ctype)
                        theirs = aten_chain(tx, tamp, iy, ix, ctype)
                        r[name + "_build"] = timed(lambda: aten_amplitudes(tr, iy, ix, ctype), args.iters)
                        r[name] = timed(lambda: aten_chain(tx, tamp, iy, ix, ctype), args.iters)
                        if kind == "f32":
                            r["max_abs_diff_" + name] = float((ours.double() - theirs.double()).abs().max())
                        else:
                            r["pixels_differing_from_" + name] = int((ours != theirs).sum())
                        r["adapt_over_" + name] = float("%.4g" % (r["adapt"]["ms"] / r[name]["ms"]))
                    except Exception as e:      # torch.fft missing or broken on this box: say so, keep our figures
                        r[name] = "torch.fft failed: %s: %s" % (type(e).__name__, str(e)[:200])
                case["radius_%d" % radius] = r
            res["%s_%dx%dx%d" % (kind, h, w, c)] = case
    r = {"batch": B, "iters": args.iters, "rounds": ROUNDS, "build": _lib.csrc_hash(), "copy_bytes_per_s": COPY_BYTES_PER_S,
         "cases": res, "clock_ghz_under_load": round(KK.clock_ghz_under_load(dev), 3)}
    print(json.dumps(r), flush=True)
    if args.out:
        with open(args.out, "w") as f:
            json.dump(r, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
