"""What the guarded optimiser steps cost (optim.py: max_grad_norm / skip_nonfinite; csrc/optim.hip: pcuda_grad_norm and the
guarded update kernels), on the real flat buffers of the default segmenter (Adam) and of one UncertaintyDiscriminator (SGD):

  (a) the unguarded step, the guarded step, and the norm launch alone -- device events around --iters calls (a spin kernel
      first, so that the host is ahead), each window --repeats times, the three alternating inside every repeat; median and
      spread (max - min).  The norm reads 4 bytes per element once: its rate is given in bytes/s beside the 6.29 TB/s this
      project quotes for a float4 copy.  No speed bar: the yardstick is the unguarded figure of the same run.
  (b) the default AdversarialTrainer.step (bench.py's full_uda: B = 32, 256 x 256, three discriminators) with the guard off
      and on (clip_gen = clip_dis = 1e30 and skip_nonfinite: every guarded kernel runs, nothing is clipped), two trainers from
      the same seed in one process, windows of --steps steps alternating, --repeats times.  The difference of the medians is
      given next to the spread of each side.

    python scripts/guarded_step_bench.py [--iters 200] [--steps 200] [--repeats 5] [--out profiles/guarded_step_bench.json]"""
import argparse
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "scripts"))
from augment_bench import device_ms  # noqa: E402
from pointcloududa_amd import _lib  # noqa: E402
from pointcloududa_amd import kernels as KK  # noqa: E402

COPY_TBS = 6.29      # float4 copy, read + write bytes per second (README)


def stats(v, digits=5):
    v = sorted(v)
    return {"ms": round(v[len(v) // 2], digits), "spread_ms": round(v[-1] - v[0], digits)}


def optimiser_level(dev, iters, repeats):
    from pointcloududa_amd.networks import Segmentation_model_Point, UncertaintyDiscriminator
    from pointcloududa_amd.optim import FusedAdam, FusedSGD
    torch.manual_seed(0)
    nets = (("segmenter_adam", Segmentation_model_Point(filters=32, in_channels=1, n_class=4, pointnet=True, fc_inch=121),
             lambda m: FusedAdam(m, lr=1e-3, betas=(0.9, 0.99), skip_prefixes=("encoder.conv1_1.",))),
            ("discriminator_sgd", UncertaintyDiscriminator(in_channel=4),
             lambda m: FusedSGD(m, lr=2.5e-5, momentum=0.99, weight_decay=0.0005)))
    res = {}
    for name, net, mk in nets:
        opt = mk(net.to(dev).train())
        opt.g.normal_(0, 1e-3)
        t = {"unguarded": [], "guarded": [], "norm_alone": []}
        for _ in range(repeats):
            opt.set_guard(0.0, False)
            t["unguarded"].append(device_ms(opt.step, iters))
            opt.set_guard(1e30, True)          # every guarded kernel runs; nothing is clipped or skipped
            t["guarded"].append(device_ms(opt.step, iters))
            t["norm_alone"].append(device_ms(lambda: opt._norm(1.0), iters))
        assert int(opt.skipped) == 0
        r = {k: stats(v) for k, v in t.items()}
        numel = opt.g.numel()
        r["numel"], r["gradient_mb"] = numel, round(4 * numel / 1e6, 2)
        r["norm_ranges"] = len(opt._norm_ranges)
        r["norm_read_tb_per_s"] = round(4 * numel / (r["norm_alone"]["ms"] * 1e-3) / 1e12, 3)
        r["norm_share_of_copy_rate"] = round(r["norm_read_tb_per_s"] / COPY_TBS, 3)
        r["guard_extra_ms"] = round(r["guarded"]["ms"] - r["unguarded"]["ms"], 5)
        res[name] = r
    return res


def trainer_level(dev, steps, repeats):
    import bench
    wl = bench.WORKLOADS["full_uda"]
    batch = bench.synth_device_batch(wl["batch"], 256, 4, 1, dev)
    trainers = {}
    for tag in ("off", "on"):
        tr = bench.build_trainer(wl, dev, 0)
        if tag == "on":
            tr.cfg.clip_gen = tr.cfg.clip_dis = 1e30
            tr.cfg.skip_nonfinite = True
            tr.apply_guard_cfg()
        for _ in range(5):
            tr.step(*batch)
        trainers[tag] = tr
    torch.cuda.synchronize()
    t = {"off": [], "on": []}
    for _ in range(repeats):
        for tag in ("off", "on"):
            tr = trainers[tag]
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            for _ in range(steps):
                out = tr.step(*batch)
            b.record()
            b.synchronize()
            t[tag].append(a.elapsed_time(b) / steps)
    assert float(out["skipped_gen"]) == 0.0 and int(trainers["on"].opt_gen.skipped) == 0
    r = {k: stats(v, 4) for k, v in t.items()}
    r["windows_ms"] = {k: [round(x, 4) for x in v] for k, v in t.items()}
    r["guard_extra_ms"] = round(r["on"]["ms"] - r["off"]["ms"], 4)
    r["guard_extra_percent"] = round(100.0 * r["guard_extra_ms"] / r["off"]["ms"], 3)
    r["img_per_s"] = {k: round(wl["batch"] / (r[k]["ms"] * 1e-3), 1) for k in ("off", "on")}
    r["workload"], r["steps_per_window"] = wl["desc"], steps
    return r


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--out", default=None, help="also write the result to this JSON file")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("guarded_step_bench: needs a HIP device")
    if args.iters < 200 or args.steps < 200:
        print("guarded_step_bench: windows shorter than 200 iterations are for rehearsal only", file=sys.stderr)
    dev = torch.device("cuda", 0)
    out = {"iters": args.iters, "repeats": args.repeats, "build": _lib.csrc_hash(),
           "figures": "median ms per call / per step; spread_ms = max - min over the repeats; unguarded, guarded and the norm "
                      "alternate inside every repeat, and so do the two trainers",
           "float4_copy_tb_per_s_quoted": COPY_TBS,
           "optimiser": optimiser_level(dev, args.iters, args.repeats),
           "trainer_step": trainer_level(dev, args.steps, args.repeats),
           "clock_ghz_under_load": round(KK.clock_ghz_under_load(dev), 3)}
    print(json.dumps(out), flush=True)
    if args.out:
        with open(args.out, "w") as f:
            json.dump(out, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
