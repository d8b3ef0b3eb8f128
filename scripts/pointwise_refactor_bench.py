"""Device time of the BatchNorm / LeakyReLU backward wrappers (kernels.py over csrc/pointwise.hip, csrc/pointnet_small.hip)
at the shapes ONE train step of ``bench.py --workload full_uda`` calls them at (B = 32, 256x256, read from a traced step:
the tables below), and the step itself, for an A/B of two builds of the library.

    python scripts/pointwise_refactor_bench.py                       # one process, the loaded library: one JSON line
    python scripts/pointwise_refactor_bench.py --ab PARENT.so --out profiles/pointwise_refactor_ab.json

``--ab``: the parent's library (``PCUDA_LIB``) and this tree's in alternation, ``--runs`` fresh processes each, then
``bench.py`` the same way.  A figure is the device time (events, the host ahead) of all the step's calls of one wrapper, each
distinct signature ``count`` times -- ms per step's worth of calls; a run's figure is its median over ``--repeats`` windows.
Bar per figure: this build's median over its runs <= the parent's median + the larger of the two builds' max - min over
their runs; the step's img/s the same way on the lower side."""
import argparse
import json
import os
import subprocess
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "scripts"))

SLOPE = 0.01
# bn_backward on planes: (shape of a / dy, second share, ntiles of red= partials from a dgrad epilogue or None, post_relu, calls)
BN_BACKWARD = (((32, 32, 256, 256), False, 2048, False, 2), ((32, 32, 256, 256), False, 1024, False, 4),
               ((32, 64, 128, 128), False, 8192, False, 2), ((32, 64, 128, 128), False, 2048, False, 4),
               ((32, 128, 64, 64), False, 2048, False, 2), ((32, 128, 64, 64), False, 512, False, 4),
               ((32, 256, 32, 32), False, 512, False, 2), ((32, 256, 32, 32), False, 128, False, 4),
               ((32, 256, 32, 32), True, None, False, 2), ((32, 128, 64, 64), True, None, False, 2),
               ((32, 64, 128, 128), True, None, False, 2),
               ((32, 128, 300), False, None, True, 6), ((32, 64, 300), False, None, True, 6))      # PointNetCls [B, C, L]
# bn_backward_pooled: (shape of a, g2, full-resolution share, calls); g / idx at half the size
BN_BACKWARD_POOLED = (((32, 32, 256, 256), True, True, 2),)
# lrelu_bwd: (shape, second share, calls); 11 x 11 planes take the flat path
LRELU_BWD = (((32, 300, 11, 11), False, 2), ((32, 512, 16, 16), False, 2), ((32, 512, 16, 16), True, 6))
# lrelu_bwd_pooled: (shape of a, g2, calls)
LRELU_BWD_POOLED = (((32, 256, 32, 32), False, 2), ((32, 128, 64, 64), True, 2), ((32, 64, 128, 128), True, 2))
# bn_backward_maxpts: (shape of a, post_relu, calls)
BN_BACKWARD_MAXPTS = (((32, 1024, 300), False, 3), ((32, 1024, 300), True, 3))
# the [B, C] pair, bn1d_forward(relu=True) and bn_backward(post_relu=True): (shape, calls of each)
BN1D = (((32, 512), 6), ((32, 256), 6))
# channel_sum: its one caller is PointNetCls.global_concat, which a full_uda step does not reach; the mmwhs_uda step's shape
CHANNEL_SUM = (((1, 16 * 1024, 300), 1),)


def figures(dev):
    """{name: fn}: each fn issues one step's worth of calls of one wrapper"""
    from pointcloududa_amd import kernels as K
    gen = torch.Generator(device=dev).manual_seed(7)
    cache = {}

    def rnd(*shape):
        return torch.randn(shape, generator=gen, device=dev)

    def layer(shape):      # a, its BatchNorm state and parameters, shared by the calls of one shape
        if shape not in cache:
            a, c = rnd(*shape), shape[1]
            gamma, beta = rnd(c), rnd(c)
            st = K.bn_finalize(*K.bn_stats(a), gamma, beta, None, None)
            cache[shape] = (a, st, gamma, torch.zeros(c, device=dev), torch.zeros(c, device=dev))
        return cache[shape]

    def half(shape):
        return shape[:2] + (shape[2] // 2, shape[3] // 2)

    jobs = {k: [] for k in ("bn_backward", "bn_backward_pooled", "lrelu_bwd", "lrelu_bwd_pooled", "bn_backward_maxpts",
                            "bn1d_pair", "channel_sum")}
    for shape, two, ntiles, pr, count in BN_BACKWARD:
        a, st, gamma, dg, db = layer(shape)
        dy, dy2 = rnd(*shape), rnd(*shape) if two else None
        red = (rnd(ntiles, shape[1], 2), ntiles) if ntiles else None
        jobs["bn_backward"].append((count, lambda a=a, st=st, gamma=gamma, dg=dg, db=db, dy=dy, dy2=dy2, red=red, pr=pr:
                                    K.bn_backward(dy, a, st, gamma, dg, db, dy2=dy2, post_relu=pr,
                                                  act_slope=1.0 if pr else SLOPE, red=red)))
    for shape, two, full, count in BN_BACKWARD_POOLED:
        a, st, gamma, dg, db = layer(shape)
        _, idx = K.maxpool2_fwd(rnd(*shape))
        g, g2, dy = rnd(*half(shape)), rnd(*half(shape)) if two else None, rnd(*shape) if full else None
        jobs["bn_backward_pooled"].append((count, lambda a=a, st=st, gamma=gamma, dg=dg, db=db, g=g, g2=g2, dy=dy, idx=idx:
                                           K.bn_backward_pooled(g, idx, a, st, gamma, dg, db, g2=g2, dy=dy, act_slope=SLOPE)))
    for shape, two, count in LRELU_BWD:
        a, dy, dy2 = rnd(*shape), rnd(*shape), rnd(*shape) if two else None
        jobs["lrelu_bwd"].append((count, lambda a=a, dy=dy, dy2=dy2: K.lrelu_bwd(dy, a, SLOPE, dy2=dy2)))
    for shape, two, count in LRELU_BWD_POOLED:
        a, g, g2 = rnd(*shape), rnd(*half(shape)), rnd(*half(shape)) if two else None
        _, idx = K.maxpool2_fwd(rnd(*shape))
        jobs["lrelu_bwd_pooled"].append((count, lambda a=a, g=g, g2=g2, idx=idx: K.lrelu_bwd_pooled(g, idx, a, SLOPE, g2=g2)))
    for shape, pr, count in BN_BACKWARD_MAXPTS:
        a, st, gamma, dg, db = layer(shape)
        _, idx = K.max_points_fwd(K.bn_apply(a, st, relu=pr))
        g = rnd(*shape[:2])
        jobs["bn_backward_maxpts"].append((count, lambda a=a, st=st, gamma=gamma, dg=dg, db=db, g=g, idx=idx, pr=pr:
                                           K.bn_backward_maxpts(g, idx, a, st, gamma, dg, db, post_relu=pr)))
    for shape, count in BN1D:
        a, dy, c = rnd(*shape), rnd(*shape), shape[1]
        gamma, beta, rm, rv, dg, db = rnd(c), rnd(c), torch.zeros(c, device=dev), torch.ones(c, device=dev), rnd(c), rnd(c)

        def pair(a=a, dy=dy, gamma=gamma, beta=beta, rm=rm, rv=rv, dg=dg, db=db):
            st, _ = K.bn1d_forward(a, gamma, beta, rm, rv, relu=True)
            K.bn_backward(dy, a, st, gamma, dg, db, post_relu=True)
        jobs["bn1d_pair"].append((count, pair))
    for shape, count in CHANNEL_SUM:
        dz, out = rnd(*shape), torch.zeros(shape[1], device=dev)
        jobs["channel_sum"].append((count, lambda dz=dz, out=out: K.channel_sum(dz, out, accumulate=False)))

    def one_step(calls):
        def run():
            for count, fn in calls:
                for _ in range(count):
                    fn()
        return run
    return {k: one_step(v) for k, v in jobs.items()}


def one_process(args):
    from augment_bench import device_ms
    from pointcloududa_amd import _lib
    from pointcloududa_amd import kernels as K
    if not torch.cuda.is_available():
        raise SystemExit("pointwise_refactor_bench: needs a HIP device")
    dev = torch.device("cuda", 0)
    out = {"build": _lib.csrc_hash(), "ms": {}}
    for name, fn in figures(dev).items():
        if args.figures and name not in args.figures.split(","):
            continue
        v = sorted(device_ms(fn, args.iters) for _ in range(args.repeats))
        out["ms"][name] = round(v[len(v) // 2], 5)
    out["clock_ghz_under_load"] = round(K.clock_ghz_under_load(dev), 3)
    print(json.dumps(out), flush=True)


def _last_json(cmd, env):
    r = subprocess.run(cmd, env=env, capture_output=True, text=True, cwd=ROOT, timeout=600)
    if r.returncode != 0:
        raise SystemExit("%s failed (%d): %s" % (" ".join(cmd), r.returncode, r.stderr[-1500:]))
    return json.loads([ln for ln in r.stdout.splitlines() if ln.startswith("{")][-1])


def _bar(parent, new, lower_is_better=True):
    med = lambda v: sorted(v)[len(v) // 2]
    margin = max(max(parent) - min(parent), max(new) - min(new))
    ok = med(new) <= med(parent) + margin if lower_is_better else med(new) >= med(parent) - margin
    return {"parent": parent, "new": new, "parent_median": med(parent), "new_median": med(new), "margin": round(margin, 5),
            "within_bar": bool(ok)}


def ab(args):
    envs = {"parent": dict(os.environ, PCUDA_LIB=os.path.abspath(args.ab)),
            "new": {k: v for k, v in os.environ.items() if k != "PCUDA_LIB"}}
    me = [sys.executable, os.path.abspath(__file__), "--iters", str(args.iters), "--repeats", str(args.repeats)]
    step = [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", str(args.steps), "--warmup", str(args.warmup)]
    runs = {"parent": [], "new": []}
    steps = {"parent": [], "new": []}
    for _ in range(args.runs):
        for side in ("parent", "new"):
            runs[side].append(_last_json(me, envs[side]))
    for _ in range(args.runs):
        for side in ("parent", "new"):
            steps[side].append(_last_json(step, envs[side]))
    builds = {side: sorted({r["build"] for r in runs[side]}) for side in runs}
    assert all(len(b) == 1 for b in builds.values()) and builds["parent"] != builds["new"], builds
    doc = {"what": __doc__.split("\n\n")[-1].replace("\n", " "),
           "builds": {side: b[0] for side, b in builds.items()},
           "clock_ghz_under_load": {side: [r["clock_ghz_under_load"] for r in runs[side]] for side in runs},
           "ms_per_steps_worth_of_calls": {name: _bar([r["ms"][name] for r in runs["parent"]], [r["ms"][name] for r in runs["new"]])
                                           for name in runs["new"][0]["ms"]},
           "step_img_per_s": _bar([r["value"] for r in steps["parent"]], [r["value"] for r in steps["new"]], lower_is_better=False),
           "step_command": "bench.py --gpus 1 --steps %d --warmup %d" % (args.steps, args.warmup)}
    doc["all_within_bar"] = all(v["within_bar"] for v in doc["ms_per_steps_worth_of_calls"].values()) and doc["step_img_per_s"]["within_bar"]
    print(json.dumps(doc), flush=True)
    if args.out:
        with open(args.out, "w") as f:
            json.dump(doc, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20, help="step's worths of calls per timed window")
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--ab", metavar="LIB", default=None, help="the parent build's libpcuda_hip.so: alternate it with this tree's")
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--steps", type=int, default=60)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--figures", default=None, help="(one process) comma-separated figure names; default all")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    ab(a) if a.ab else one_process(a)
