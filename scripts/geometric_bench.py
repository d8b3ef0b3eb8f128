"""Device time per call of the device-side geometric augmentation (utils/geometric.py, csrc/geometric.hip),
B = 32, 256x256x3 uint8 images (6.3 MB) with int32 labels (8.4 MB):

  (a) each opcode alone (one slot, every sample the same encoder; with and without labels), next to a uint8 copy of the
      image bytes by torch (the byte bound f7 used: 6.3 MB read + 6.3 MB written) and the one-slot NOP program
  (b) a sampled "heavy_device" plan (photometric and geometric stages) and its geometric stages alone
  (c) augment_batch (identity parameters, /255, crop 224) with and without the plan, as a loader calls it (c_call*:
      programs validated and uploaded per call, where the host's issue time shows), and the extra pass that fusing the
      last geometric slot into augment_assemble would save: the one-slot NOP program with labels
  (d) the host time of sample_heavy_plan per batch
  (e) the plain-numpy and the scipy restatement of the plan's geometric stages on this machine's host CPU
      (scripts/make_geometric_golden.py)

(a), (b) are timed with the host running ahead of the device (a spin kernel goes first).

    python scripts/geometric_bench.py [--iters 100] [--out profiles/geometric_bench.json]

``--cubic`` (f8b) measures something else and nothing of the above: per opcode, with labels, the order-1 row through
``pcuda_geometric`` (the kernel instance that serves orders 0 and 1), the same order-1 program through ``pcuda_geometric_cubic``
(what the second instance costs a program without order 3, which ``geometric_aug`` never sends there) and the order-3 row, ``--runs``
times over; the result goes under the key ``"geometric"`` of ``--out`` (other keys of an existing file are kept:
``stylize_bench.py --cubic`` writes its own into the same file).

    python scripts/geometric_bench.py --cubic [--runs 5] [--out profiles/geometric_cubic_bench.json]"""
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
import make_geometric_golden as G  # noqa: E402
import make_photometric_golden as PG  # noqa: E402
from augment_bench import device_ms  # noqa: E402
from oracle.synth import synth_batch  # noqa: E402
from pointcloududa_amd import _lib  # noqa: E402
from pointcloududa_amd import kernels as KK  # noqa: E402
from pointcloududa_amd.utils import geometric as P  # noqa: E402
from pointcloududa_amd.utils import photometric as F7  # noqa: E402
from pointcloududa_amd.utils.augment import augment_batch, heavy_aug, sample_heavy_plan  # noqa: E402

B, H, W, C, K = 32, 256, 256, 3, 5
PRESET = "heavy_device"


def one_op(setter, *args, **kw):
    prog = P.GeoProgram.identity(B, 1)
    for i in range(B):
        getattr(prog, setter)(i, 0, *args, **kw)
    return prog


def host_ms(fn, reps):
    fn()
    t0 = time.perf_counter()
    for _ in range(reps):
        fn()
    return 1e3 * (time.perf_counter() - t0) / reps


def order_rows():
    """name -> order-1 program of one opcode, every sample the same encoder (the rows of --cubic)"""
    rng = np.random.default_rng(7)
    jit = rng.normal(0, 0.1, (4, 2)).clip(-0.45, 0.45)
    dx, dy = rng.normal(0, 0.05 * W, (4, 4)), rng.normal(0, 0.05 * H, (4, 4))
    aff = dict(scale_x=0.8, scale_y=1.2, translate_x=0.2, translate_y=-0.2, rotate=45.0, shear=16.0)
    return {
        "affine_constant": one_op("set_affine", H, W, order=1, mode=0, cval=7, **aff),
        "affine_reflect": one_op("set_affine", H, W, order=1, mode=2, **aff),
        "affine_wrap": one_op("set_affine", H, W, order=1, mode=4, **aff),
        "crop_and_pad": one_op("set_crop_and_pad", H, W, 26, -13, 25, -12, 3, 0),
        "perspective": one_op("set_perspective", H, W, jit),
        "elastic_r1": one_op("set_elastic", 3.5, 0.25, 1234567),
        "elastic_r4": one_op("set_elastic", 20.0, 1.0, 1234567),
        "piecewise_g4": one_op("set_piecewise", H, W, dx, dy),
    }


def merge_out(path, key, value):
    """write ``value`` under ``key`` of the JSON file ``path``, keeping its other keys"""
    doc = {}
    if os.path.exists(path):
        with open(path) as f:
            doc = json.load(f)
    doc[key] = value
    with open(path, "w") as f:
        json.dump(doc, f, indent=1)
        f.write("\n")


def cubic_main(args, dev):
    x = np.concatenate([PG.make_images("grey3", 16, H, W, C, 71), PG.make_images("smooth", 8, H, W, C, 72),
                        PG.make_images("random", 8, H, W, C, 73)])
    lab = np.argmax(synth_batch(B, 1, K, H, seed=3)[1], axis=1).astype(np.int32)
    tx, tl32 = torch.from_numpy(x).to(dev), torch.from_numpy(lab).to(dev)
    out, out_lab = torch.empty_like(tx), torch.empty_like(tl32)
    rows = {}
    for name, prog in order_rows().items():
        up1 = P.upload_geo_program(prog, B, H, W, dev)
        prog.iarg[..., 0] = 3
        up3 = P.upload_geo_program(prog, B, H, W, dev)
        rows[name + "_order1"] = (up1, False)
        rows[name + "_order1_cubic_entry"] = (up1, True)
        rows[name + "_order3"] = (up3, True)
    runs = []
    for _ in range(args.runs):
        runs.append({name: round(device_ms(lambda: KK.geometric(tx, tl32, *up, out=out, labels_out=out_lab, cubic=cubic), args.iters), 4)
                     for name, (up, cubic) in rows.items()})
    r = {"shape": [B, H, W, C], "iters": args.iters, "build": _lib.csrc_hash(), "with_labels": True, "runs_ms": runs,
         "median_ms": {k: round(float(np.median([q[k] for q in runs])), 4) for k in runs[0]},
         "min_max_ms": {k: [min(q[k] for q in runs), max(q[k] for q in runs)] for k in runs[0]},
         "clock_ghz_under_load": round(KK.clock_ghz_under_load(dev), 3)}
    print(json.dumps(r), flush=True)
    if args.out:
        merge_out(args.out, "geometric", r)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=100)
    ap.add_argument("--out", default=None, help="also write the result to this JSON file")
    ap.add_argument("--cubic", action="store_true", help="order-1 against order-3 rows per opcode (f8b) and nothing else")
    ap.add_argument("--runs", type=int, default=5, help="--cubic: how often every row is measured")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("geometric_bench: needs a HIP device")
    dev = torch.device("cuda", 0)
    if args.cubic:
        return cubic_main(args, dev)
    x = np.concatenate([PG.make_images("grey3", 16, H, W, C, 71), PG.make_images("smooth", 8, H, W, C, 72),
                        PG.make_images("random", 8, H, W, C, 73)])
    lab = np.argmax(synth_batch(B, 1, K, H, seed=3)[1], axis=1).astype(np.int64)
    tx, tl = torch.from_numpy(x).to(dev), torch.from_numpy(lab).to(dev)
    tl32 = tl.to(torch.int32)
    nbytes = 2 * x.size
    out, out_lab = torch.empty_like(tx), torch.empty_like(tl32)

    def timed(prog, labels=True):
        up = P.upload_geo_program(prog, B, H, W, dev)
        if labels:
            return device_ms(lambda: KK.geometric(tx, tl32, *up, out=out, labels_out=out_lab), args.iters)
        return device_ms(lambda: KK.geometric(tx, None, *up, out=out), args.iters)
    rng = np.random.default_rng(7)
    jit = rng.normal(0, 0.1, (4, 2)).clip(-0.45, 0.45)
    dx, dy = rng.normal(0, 0.05 * W, (4, 4)), rng.normal(0, 0.05 * H, (4, 4))
    aff = dict(scale_x=0.8, scale_y=1.2, translate_x=0.2, translate_y=-0.2, rotate=45.0, shear=16.0)
    ops = {
        "nop": P.GeoProgram.identity(B, 1),
        "flip_lr": one_op("set_flip_lr", W),
        "affine_order0_constant": one_op("set_affine", H, W, order=0, mode=0, cval=7, **aff),
        "affine_order1_constant": one_op("set_affine", H, W, order=1, mode=0, cval=7, **aff),
        "affine_order1_reflect": one_op("set_affine", H, W, order=1, mode=2, **aff),
        "affine_order1_wrap": one_op("set_affine", H, W, order=1, mode=4, **aff),
        "crop_and_pad": one_op("set_crop_and_pad", H, W, 26, -13, 25, -12, 3, 0),
        "perspective": one_op("set_perspective", H, W, jit),
        "elastic_r1": one_op("set_elastic", 3.5, 0.25, 1234567),
        "elastic_r4": one_op("set_elastic", 20.0, 1.0, 1234567),
        "piecewise_g4": one_op("set_piecewise", H, W, dx, dy),
    }
    a_ms = {"torch_copy": device_ms(lambda: out.copy_(tx), args.iters)}
    a_nolab = {}
    for name, prog in ops.items():
        a_ms[name] = timed(prog)
        a_nolab[name] = timed(prog, labels=False)

    plan = sample_heavy_plan(B, PRESET, np.random.default_rng(2027), H, W)
    geo = [st for st in plan.stages if isinstance(st, P.GeoProgram)]
    ups = [(isinstance(st, P.GeoProgram), P.upload_geo_program(st, B, H, W, dev) if isinstance(st, P.GeoProgram)
            else F7.upload_program(st, B, H, W, C, dev)) for st in plan.stages]

    def run_plan(only_geo=False):
        cx, cl = tx, tl32
        for is_geo, up in ups:
            if is_geo:
                cx, cl = KK.geometric(cx, cl, *up)
            elif not only_geo:
                cx = KK.photometric(cx, *up)
        return cx, cl
    b_ms = {"plan": device_ms(run_plan, args.iters), "plan_geometric_stages": device_ms(lambda: run_plan(True), args.iters)}

    c_ms = {
        "c_call": device_ms(lambda: augment_batch(tx, tl, None, K, 224, rescale="div255"), args.iters, ahead=False),
        "c_call_heavy": device_ms(lambda: augment_batch(tx, tl, None, K, 224, rescale="div255", heavy=plan), args.iters, ahead=False),
        "c_call_heavy_ahead": device_ms(lambda: augment_batch(tx, tl, None, K, 224, rescale="div255", heavy=plan), args.iters),
        "heavy_aug": device_ms(lambda: heavy_aug(tx, tl, plan), args.iters, ahead=False),
        "extra_pass_nop_with_labels": a_ms["nop"],
    }
    rng = np.random.default_rng(5)
    d_ms = {"sample_heavy_plan": host_ms(lambda: sample_heavy_plan(B, PRESET, rng, H, W), 50)}
    torch.cuda.synchronize()

    def restate(backend):
        cx, cl = x, lab
        for st in geo:
            cx, cl = G.run_program(cx, cl, st.opcode, st.iarg, st.farg, st.seed, backend=backend)[:2]
    e_ms = {"numpy": host_ms(lambda: restate("numpy"), 2)}
    try:
        import scipy  # noqa: F401
        e_ms["scipy"] = host_ms(lambda: restate("scipy"), 2)
    except ImportError:
        e_ms["scipy"] = None
    rnd = lambda d: {k: (None if v is None else round(v, 4)) for k, v in d.items()}
    step_ms = (41.0, 44.0)      # the training step these batches hide behind (profiles)
    two = 2.0 * c_ms["c_call_heavy_ahead"]
    r = {"shape": [B, H, W, C], "iters": args.iters, "build": _lib.csrc_hash(), "copy_bytes": nbytes,
         "a_ms_with_labels": rnd(a_ms), "a_ms_images_only": rnd(a_nolab),
         "a_over_torch_copy": {k: round(v / a_ms["torch_copy"], 2) for k, v in a_ms.items()},
         "b_ms": rnd(b_ms), "b_stages": [[type(st).__name__, int(st.slots), int((st.opcode != 0).sum())] for st in plan.stages],
         "b_geo_opcodes": {P.OP_NAMES[c]: int(sum((st.opcode == c).sum() for st in geo)) for c in range(1, 4)},
         "clock_ghz_under_load": round(KK.clock_ghz_under_load(dev), 3), "c_ms": rnd(c_ms),
         "two_domains_share_of_step": [round(two / s, 4) for s in step_ms[::-1]],
         "d_host_ms": rnd(d_ms), "e_host_ms": rnd(e_ms), "host_threads": os.environ.get("OMP_NUM_THREADS")}
    print(json.dumps(r), flush=True)
    if args.out:
        with open(args.out, "w") as f:
            json.dump(r, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
