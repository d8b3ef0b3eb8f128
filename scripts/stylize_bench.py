"""Device time per call of the device-side stylize augmentation (utils/stylize.py, csrc/stylize.hip), B = 32, 256x256x3 uint8
(6.3 MB):

  (a) each operator alone (one slot, every sample the same opcode): hue / saturation, noise-alpha at its two ends (one 2x2
      grid, nearest, no sigmoid; three 16x16 grids, bilinear, mean, sigmoid), superpixels at n_segments = 20 and 200 (5 updates)
      and at 200 without updates, next to a uint8 copy of the same bytes by torch (the byte bound) and the one-slot NOP program
  (b) a sampled "heavy_full_device" plan through heavy_aug's kernels (programs already on the device), and its stylize
      stages alone
  (c) augment_batch (mscmrseg_simple, /255, crop 224) as a loader calls it, with and without the plan (parameters composed,
      validated and uploaded per call, where the host's issue time shows)
  (d) the host time of sample_heavy_plan for the full and for the f8 preset (the difference holds the simplex grids), and of
      sampling + uploading
  (e) the numpy restatement of the plan's stylize stages on this machine's host CPU (scripts/make_stylize_golden.py)

(a) and (b) are timed with the host running ahead of the device (a spin kernel goes first).

    python scripts/stylize_bench.py [--iters 100] [--out profiles/stylize_bench.json]

``--cubic`` (f8b) measures the noise-alpha slot alone -- one 2x2 grid and three 16x16 grids (mean, sigmoid), each with the
bilinear and with the cubic upscale -- ``--runs`` times over and writes it under the key ``"stylize"`` of ``--out`` (other keys of
an existing file are kept: ``geometric_bench.py --cubic`` writes its own into the same file).

    python scripts/stylize_bench.py --cubic [--runs 5] [--out profiles/geometric_cubic_bench.json]"""
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
import make_stylize_golden as G  # noqa: E402
from augment_bench import device_ms  # noqa: E402
from oracle.synth import synth_batch  # noqa: E402
from pointcloududa_amd import _lib  # noqa: E402
from pointcloududa_amd import kernels as KK  # noqa: E402
from pointcloududa_amd.utils import geometric as Geo  # noqa: E402
from pointcloududa_amd.utils import photometric as P  # noqa: E402
from pointcloududa_amd.utils import stylize as S  # noqa: E402
from pointcloududa_amd.utils.augment import augment_batch, sample_heavy_plan, sample_params  # noqa: E402

B, H, W, C, K = 32, 256, 256, 3, 5
PRESET = "heavy_full_device"


def one_op(setter, *args, **kw):
    prog = S.StyleProgram.identity(B, 1)
    for i in range(B):
        getattr(prog, setter)(i, 0, *args, **kw)
    return prog


def host_ms(fn, reps):
    fn()
    t0 = time.perf_counter()
    for _ in range(reps):
        fn()
    return 1e3 * (time.perf_counter() - t0) / reps


def cubic_main(args, dev):
    from geometric_bench import merge_out
    x = np.concatenate([G.make_images("grey3", 16, H, W, C, 71), G.make_images("smooth", 8, H, W, C, 72),
                        G.make_images("random", 8, H, W, C, 73)])
    tx = torch.from_numpy(x).to(dev)
    out = torch.empty_like(tx)
    small = [S.simplex_grid(2, 2, 5)]
    large = [S.simplex_grid(16, 16, 5 + k) for k in range(3)]
    rows = {}
    for up_name, up_mode in (("bilinear", S.UPSCALE_BILINEAR), ("cubic", S.UPSCALE_CUBIC)):
        rows["noise_alpha_1x2x2_%s" % up_name] = one_op("set_noise_alpha", S.edge_detect_weights(0.8), small, up_mode, S.AGG_MIN, False, 0.0)
        rows["noise_alpha_3x16x16_%s_sigmoid" % up_name] = one_op("set_noise_alpha", S.directed_edge_weights(0.8, 0.3), large, up_mode,
                                                                  S.AGG_MEAN, True, 1.0)
    ups = {name: S.upload_style_program(prog, B, H, W, C, dev) for name, prog in rows.items()}
    runs = [{name: round(device_ms(lambda: KK.stylize(tx, *up, out=out), args.iters), 4) for name, up in ups.items()}
            for _ in range(args.runs)]
    r = {"shape": [B, H, W, C], "iters": args.iters, "build": _lib.csrc_hash(), "runs_ms": runs,
         "median_ms": {k: round(float(np.median([q[k] for q in runs])), 4) for k in runs[0]},
         "min_max_ms": {k: [min(q[k] for q in runs), max(q[k] for q in runs)] for k in runs[0]}}
    print(json.dumps(r), flush=True)
    if args.out:
        merge_out(args.out, "stylize", r)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=100)
    ap.add_argument("--out", default=None, help="also write the result to this JSON file")
    ap.add_argument("--cubic", action="store_true", help="the noise-alpha slot, bilinear against cubic (f8b), and nothing else")
    ap.add_argument("--runs", type=int, default=5, help="--cubic: how often every row is measured")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("stylize_bench: needs a HIP device")
    dev = torch.device("cuda", 0)
    if args.cubic:
        return cubic_main(args, dev)
    x = np.concatenate([G.make_images("grey3", 16, H, W, C, 71), G.make_images("smooth", 8, H, W, C, 72),
                        G.make_images("random", 8, H, W, C, 73)])
    lab = np.argmax(synth_batch(B, 1, K, H, seed=3)[1], axis=1).astype(np.int64)
    tx, tl = torch.from_numpy(x).to(dev), torch.from_numpy(lab).to(dev)
    tl32 = tl.to(torch.int32)
    nbytes = 2 * x.size
    out = torch.empty_like(tx)

    def timed(prog):
        up = S.upload_style_program(prog, B, H, W, C, dev)
        return device_ms(lambda: KK.stylize(tx, *up, out=out), args.iters)
    small = [S.simplex_grid(2, 2, 5)]
    large = [S.simplex_grid(16, 16, 5 + k) for k in range(3)]
    ops = {
        "torch_copy": None,
        "nop": S.StyleProgram.identity(B, 1),
        "hue_saturation": one_op("set_hue_saturation", 14, 20),
        "noise_alpha_1x2x2_nearest": one_op("set_noise_alpha", S.edge_detect_weights(0.8), small, S.UPSCALE_NEAREST, S.AGG_MIN, False, 0.0),
        "noise_alpha_3x16x16_bilinear_sigmoid": one_op("set_noise_alpha", S.directed_edge_weights(0.8, 0.3), large, S.UPSCALE_BILINEAR,
                                                       S.AGG_MEAN, True, 1.0),
        "superpixels_n20": one_op("set_superpixels", *S.superpixel_grid(20, H, W), 0.7, 1234567),
        "superpixels_n200": one_op("set_superpixels", *S.superpixel_grid(200, H, W), 0.7, 1234567),
        "superpixels_n200_no_update": one_op("set_superpixels", *S.superpixel_grid(200, H, W), 0.7, 1234567, iters=0),
    }
    a_ms = {}
    for name, prog in ops.items():
        a_ms[name] = device_ms(lambda: out.copy_(tx), args.iters) if prog is None else timed(prog)

    plan = sample_heavy_plan(B, PRESET, np.random.default_rng(2029), H, W)
    ups = []
    for st in plan.stages:
        if isinstance(st, S.StyleProgram):
            ups.append(("s", S.upload_style_program(st, B, H, W, C, dev)))
        elif isinstance(st, P.PhotoProgram):
            ups.append(("p", P.upload_program(st, B, H, W, C, dev)))
        else:
            ups.append(("g", Geo.upload_geo_program(st, B, H, W, dev)))

    def run_plan(only=None):
        img, lb = tx, tl32
        for kind, up in ups:
            if only and kind != only:
                continue
            if kind == "s":
                img = KK.stylize(img, *up)
            elif kind == "p":
                img = KK.photometric(img, *up)
            else:
                img, lb = KK.geometric(img, lb, *up)
        return img
    b_ms = {"plan_kernels": device_ms(run_plan, args.iters), "plan_stylize_stages_only": device_ms(lambda: run_plan("s"), args.iters)}
    style = [st for st in plan.stages if isinstance(st, S.StyleProgram)]
    b_slots = {"stages": [type(st).__name__ + ":%d" % st.slots for st in plan.stages],
               "stylize_opcodes": {S.OP_NAMES[c]: int(sum((st.opcode == c).sum() for st in style)) for c in range(1, 4)}}

    params = sample_params(B, "mscmrseg_simple", np.random.default_rng(1))
    c_ms = {"c_call": device_ms(lambda: augment_batch(tx, tl, params, K, 224, rescale="div255"), args.iters, ahead=False),
            "c_call_full_plan": device_ms(lambda: augment_batch(tx, tl, params, K, 224, rescale="div255", heavy=plan), args.iters, ahead=False)}
    rng = np.random.default_rng(5)

    def sample_and_upload():
        for st in sample_heavy_plan(B, PRESET, rng, H, W).stages:
            if isinstance(st, S.StyleProgram):
                S.upload_style_program(st, B, H, W, C, dev)
            elif isinstance(st, P.PhotoProgram):
                P.upload_program(st, B, H, W, C, dev)
            else:
                Geo.upload_geo_program(st, B, H, W, dev)
    d_ms = {"sample_heavy_plan_full": host_ms(lambda: sample_heavy_plan(B, PRESET, rng, H, W), 30),
            "sample_heavy_plan_f8": host_ms(lambda: sample_heavy_plan(B, "heavy_device", rng, H, W), 30),
            "simplex_grid_16x16": host_ms(lambda: S.simplex_grid(16, 16, 7), 200),
            "sample_and_upload_full": host_ms(sample_and_upload, 30)}
    torch.cuda.synchronize()

    def restate():
        cur = x
        for st in style:
            cur = G.run_program(cur, st.opcode, st.iarg, st.farg, st.table, st.seed, backend="numpy")[0]
    e_ms = {"numpy_stylize_stages": host_ms(restate, 2)}
    rnd = lambda d: {k: (None if v is None else round(v, 4)) for k, v in d.items()}
    r = {"shape": [B, H, W, C], "iters": args.iters, "build": _lib.csrc_hash(), "copy_bytes": nbytes,
         "a_ms": rnd(a_ms), "a_over_torch_copy": {k: round(v / a_ms["torch_copy"], 2) for k, v in a_ms.items()},
         "b_ms": rnd(b_ms), "b_plan": b_slots, "clock_ghz_under_load": round(KK.clock_ghz_under_load(dev), 3), "c_ms": rnd(c_ms),
         "two_domains_share_of_step": {"step_ms": [41.0, 44.0],
                                       "share": [round(2 * c_ms["c_call_full_plan"] / 44.0, 4), round(2 * c_ms["c_call_full_plan"] / 41.0, 4)]},
         "d_host_ms": rnd(d_ms), "e_host_ms": rnd(e_ms), "host_threads": os.environ.get("OMP_NUM_THREADS")}
    print(json.dumps(r), flush=True)
    if args.out:
        with open(args.out, "w") as f:
            json.dump(r, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
