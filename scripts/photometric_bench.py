"""Device time per call of the device-side photometric augmentation (utils/photometric.py, csrc/photometric.hip),
B = 32, 256x256x3 uint8 (6.3 MB):

  (a) each operator alone (one slot, every sample the same opcode) at its most expensive parameter (sigma = 3, average
      k = 7, median k = 11), next to a uint8 copy of the same bytes by torch (the byte bound: 6.3 MB read + 6.3 MB written)
      and the one-slot NOP program (the copy through this library's pointwise kernel)
  (b) a sampled five-slot "mscmrseg_aug2_photometric" program
  (c) augment_batch (mscmrseg_simple, /255, crop 224) with and without the program: at the kernel wrappers with the
      parameters already on the device (c_kernels*), and as a loader calls it (c_call*: parameters composed, validated and
      uploaded per call, where the host's issue time shows)
  (d) the host time of sample_program + upload_program per batch
  (e) the plain-numpy and the scipy restatement of (b) on this machine's host CPU (scripts/make_photometric_golden.py)

(a), (b) and c_kernels* are timed with the host running ahead of the device (a spin kernel goes first).

    python scripts/photometric_bench.py [--iters 200] [--out profiles/photometric_bench.json]"""
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
import make_photometric_golden as G  # noqa: E402
from augment_bench import device_ms  # noqa: E402
from oracle.synth import synth_batch  # noqa: E402
from pointcloududa_amd import _lib  # noqa: E402
from pointcloududa_amd import kernels as KK  # noqa: E402
from pointcloududa_amd.utils import photometric as P  # noqa: E402
from pointcloududa_amd.utils.augment import augment_batch, sample_params, upload_params  # noqa: E402

B, H, W, C, K = 32, 256, 256, 3, 5
PRESET = "mscmrseg_aug2_photometric"


def one_op(setter, *args):
    prog = P.PhotoProgram.identity(B, 1)
    for i in range(B):
        getattr(prog, setter)(i, 0, *args)
    return prog


def host_ms(fn, reps):
    fn()
    t0 = time.perf_counter()
    for _ in range(reps):
        fn()
    return 1e3 * (time.perf_counter() - t0) / reps


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--out", default=None, help="also write the result to this JSON file")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("photometric_bench: needs a HIP device")
    dev = torch.device("cuda", 0)
    x = np.concatenate([G.make_images("grey3", 16, H, W, C, 71), G.make_images("smooth", 8, H, W, C, 72),
                        G.make_images("random", 8, H, W, C, 73)])
    lab = np.argmax(synth_batch(B, 1, K, H, seed=3)[1], axis=1).astype(np.int64)
    tx, tl = torch.from_numpy(x).to(dev), torch.from_numpy(lab).to(dev)
    tl32 = tl.to(torch.int32)
    nbytes = 2 * x.size
    out = torch.empty_like(tx)

    def timed(prog):
        up = P.upload_program(prog, B, H, W, C, dev)
        return device_ms(lambda: KK.photometric(tx, *up, out=out), args.iters)
    ops = {
        "torch_copy": None,
        "nop": P.PhotoProgram.identity(B, 1),
        "gaussian_blur_sigma3": one_op("set_gaussian_blur", 3.0),
        "average_blur_k7": one_op("set_average_blur", 7),
        "median_blur_k11": one_op("set_median_blur", 11),
        "median_blur_k3": one_op("set_median_blur", 3),
        "conv3x3": one_op("set_conv3x3", P.sharpen_weights(0.7, 1.2)),
        "gaussian_noise": one_op("set_gaussian_noise", 12.0, True, 1234567),
        "dropout": one_op("set_dropout", 0.1, True, 1234567),
        "coarse_dropout": one_op("set_coarse_dropout", 0.15, 0.05, True, 1234567),
        "invert": one_op("set_invert", (1, 0, 1)),
        "add": one_op("set_add", (10, -10, 3)),
        "multiply": one_op("set_multiply", (0.7, 1.3, 1.1)),
        "grayscale": one_op("set_grayscale", 0.6),
    }
    a_ms = {}
    for name, prog in ops.items():
        a_ms[name] = device_ms(lambda: out.copy_(tx), args.iters) if prog is None else timed(prog)
    prog = P.sample_program(B, PRESET, np.random.default_rng(2026))
    b_ms = timed(prog)

    params = sample_params(B, "mscmrseg_simple", np.random.default_rng(1))
    up_a, up_p = upload_params(params, B, H, W, dev), P.upload_program(prog, B, H, W, C, dev)
    c_ms = {
        "c_kernels": device_ms(lambda: KK.augment_assemble(tx, tl32, *up_a, K, 224, KK.AUG_DIV255), args.iters),
        "c_kernels_photometric": device_ms(
            lambda: KK.augment_assemble(KK.photometric(tx, *up_p, out=out), tl32, *up_a, K, 224, KK.AUG_DIV255), args.iters),
        "c_call": device_ms(lambda: augment_batch(tx, tl, params, K, 224, rescale="div255"), args.iters, ahead=False),
        "c_call_photometric": device_ms(lambda: augment_batch(tx, tl, params, K, 224, rescale="div255", photometric=prog),
                                        args.iters, ahead=False),
    }
    rng = np.random.default_rng(5)
    d_ms = {"sample_program": host_ms(lambda: P.sample_program(B, PRESET, rng), 50),
            "sample_and_upload": host_ms(lambda: P.upload_program(P.sample_program(B, PRESET, rng), B, H, W, C, dev), 50)}
    torch.cuda.synchronize()
    e_ms = {"numpy": host_ms(lambda: G.run_program(x, prog.opcode, prog.iarg, prog.farg, prog.seed, backend="numpy"), 2)}
    try:
        import scipy  # noqa: F401
        e_ms["scipy"] = host_ms(lambda: G.run_program(x, prog.opcode, prog.iarg, prog.farg, prog.seed, backend="scipy"), 2)
    except ImportError:
        e_ms["scipy"] = None
    rnd = lambda d: {k: (None if v is None else round(v, 4)) for k, v in d.items()}
    r = {"shape": [B, H, W, C], "iters": args.iters, "build": _lib.csrc_hash(), "copy_bytes": nbytes,
         "a_ms": rnd(a_ms), "a_over_torch_copy": {k: round(v / a_ms["torch_copy"], 2) for k, v in a_ms.items()},
         "a_gbps": {k: round(nbytes / (v * 1e6), 1) for k, v in a_ms.items()},
         "b_ms": round(b_ms, 4), "b_active_slots": int((prog.opcode != 0).sum()),
         "b_opcodes": {P.OP_NAMES[c]: int((prog.opcode == c).sum()) for c in range(1, 12)},
         "clock_ghz_under_load": round(KK.clock_ghz_under_load(dev), 3), "c_ms": rnd(c_ms), "d_host_ms": rnd(d_ms), "e_host_ms": rnd(e_ms), "host_threads": os.environ.get("OMP_NUM_THREADS")}
    print(json.dumps(r), flush=True)
    if args.out:
        with open(args.out, "w") as f:
            json.dump(r, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
