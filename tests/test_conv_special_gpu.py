"""The purpose-built convolution kernels -- anti-phase (conv3ap), row-streaming (conv3rs), wgrad3, wgrad3r, wgrad1 and the direct
kernels, none of which has a variant key (tests/test_conv_variants_gpu.py sweeps the keyed ones) -- against the operand-exact
reference of tests/conv_exact_ref.py, attributed instantiation by instantiation through the launch tag.

The sweep runs in child processes (tests/conv_special_child.py, one per table, one after the other: PCUDA_WGRAD3R and
PCUDA_W3_MINCOUT are read once per process).  Per operation: the launch tag names the intended kernel, ``fallback_count()`` did
not move, and all it computed is within BOTH bounds -- 4 x chains x e32 per output channel (``axis=0`` for weight gradients;
per-channel sums against the channel's sum of |terms|) against the operand-exact float64 reference, e32 = the same expression
in float32 on the CPU, chains = 3 in bf16x3 mode, 1 in bf16 mode and for the direct kernels (fp32 FMA on unrounded
activations) -- and the project's old bound on the whole tensor.

INSTANTIATIONS lists what the launch switch statements can start: conv3rs 12 = STATS {0, 1, 2} x ACC x AFF (csrc/conv_rs.hip:441-444),
conv3ap 8 (csrc/conv_ap.hip:176-183), wgrad3r {bf16, bf16x3} x {plain, UP} (csrc/conv_wgrad3r.hip:410-415), wgrad3 per precision
(csrc/conv_wgrad3.hip:431-432), wgrad1 per precision x co_b {1, 2} x ci_b {1, 2, 3} (csrc/conv_wgrad1.hip:284-289), and the direct
kernels behind the seven PCUDA_DIRECT_MASK bits (+ the 1x1 data gradient with the fused reduce, + d1_fwd_kernel) per precision.
UNREACHABLE, one entry per kernel file: STATS = 1 (the forward's sum / sum of squares) with ACC -- ``pcuda_conv2d_forward`` sets
``accumulate = 0`` (csrc/conv_igemm.hip:617) and is the only entry point that passes ``bn_partials`` without ``red_a``, so
conv3ap<1, true> and conv3rs<1, true, AFF> (both AFF: the one condition forbids the pair) are built and never launched.

MECHANISMS: the plan branches behind one instantiation that the cases were chosen for, read back from the tags.

Measured on an MI355X, largest kernel error / e32 over every check of every operation (the kernels are deterministic: the
figures repeat run to run):
    kernel     bf16 (bound 4)   bf16x3 (bound 12)
    conv3ap    -                7.17   (a BatchNorm-backward partial sum behind the 2x2 fold; convolution outputs 4.78)
    conv3rs    -                6.11   (a BatchNorm-backward partial sum, 4 x 64 x 128; convolution outputs below 3)
    wgrad3     1.42             1.42   (the bias gradient in both; the weight gradients lie below it)
    wgrad3r    1.47             1.47   (the same)
    wgrad1     1.00             1.97
    direct     2.61 (bound 4)   1.82 (bound 4: one chain in both modes)
Nothing exceeded the bound and no kernel needed a fix; no factor beyond 4 x chains was needed either -- conv3rs adds a lane's
partial sums sequentially over its strip (csrc/conv_rs.hip:213-214) where torch's float32 ``sum`` is pairwise, and stays at 6.1
of 12 (256 to 304 additions per lane in the cases with the largest ratios).
Wall time of the three children on that machine: 8.9 s together (ap_rs 4.2 s, of which 2.2 s in the sweep -- the float64
references; w3_w1_direct 2.2 s and w3r 2.5 s, 0.3-0.4 s in the sweep, the rest starting Python and loading the library).
CHILD_TIMEOUT is a hang guard of more than a hundred times the slowest child.

Self-check (scratch copies, not committed; one build and one run each, this file and today's tests of the kernel):
  1. conv3rs, the halo pixel's lo plane zeroed (``cL.x = 0`` at csrc/conv_rs.hip:180: the xl x wh plane of the pixel beside the
     strip): all ten reachable conv3rs instantiations and the all-operations test fail here, e.g. forward 2 x 19 x 96: error
     1.24e-3 of the channel, 4809 x e32 against the bound of 12.  Today's tests/test_conv_rs_gpu.py fails as well (11 of 15: 5.2e-4
     ... 1.1e-3 against 1e-4): with 96 of a pixel's 288 products affected the old bound sees it.  The same for channel 31's right
     halo pixel only: 919 x e32 here, 1.6e-4 ... 3.6e-4 against 1e-4 there -- in this kernel a dropped lo plane does not pass
     today's bound even on one channel of one halo column (3 of 288 products at 2^-9: about 2e-4 of the output).
  2. wgrad1 in bf16 mode, input channel 31 of every 32-block scaled by 0.999 at the slab store (csrc/conv_wgrad1.hip:194): the
     five wgrad1-bf16 instantiations that had a channel 31 and the all-operations test fail here (errors 8.9e-4 ... 1.03e-3 of a
     row against bounds of 4.8e-7 ... 1.4e-6: 3000 ... 7400 x e32) while all ten cases of
     test_conv_gpu.py::test_pointwise_layer_weight_gradient_from_global_rows pass (2.2e-3 ... 3.6e-3 against 2e-2).  The sixth,
     co1-ci1, had only the ragged 20 -> 24 case then and passed: the full 32 -> 32 case was added for it.
"""
import json
import os
import subprocess
import sys
import time

import pytest

from conv_special_child import TABLES, inst_of, tag_int

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
CHILD = os.path.join(HERE, "conv_special_child.py")
CHILD_TIMEOUT = 600    # seconds; a hang guard, not a budget

BOTH = ("bf16x3", "bf16")
INSTANTIATIONS = (
    ["conv3rs-stats%d-acc%d-aff%d" % (s, a, f) for s in (0, 1, 2) for a in (0, 1) for f in (0, 1)] +
    ["conv3ap-stats%d-acc%d-fold0" % (s, a) for s in (0, 1, 2) for a in (0, 1)] + ["conv3ap-stats0-acc0-fold1", "conv3ap-stats2-acc0-fold1"] +
    ["wgrad3r-%s-up%d" % (p, u) for p in BOTH for u in (0, 1)] +
    ["wgrad3-%s" % p for p in BOTH] +
    ["wgrad1-%s-co%d-ci%d" % (p, co, ci) for p in BOTH for co in (1, 2) for ci in (1, 2, 3)] +
    ["direct-%s-%s" % (k, p) for k in ("c1-fwd", "c1-wgrad", "1x1-fwd", "1x1-dgrad", "1x1-dgrad+bnred", "d1-dgrad", "d1-wgrad", "d5-fwd", "d1-fwd")
     for p in BOTH])
# (kernel file, instantiations, the dispatcher condition that forbids them): at most one entry per kernel file
UNREACHABLE = [
    ("conv_rs.hip", ("conv3rs-stats1-acc1-aff0", "conv3rs-stats1-acc1-aff1"),
     "STATS 1 comes from pcuda_conv2d_forward alone, which sets accumulate = 0 (conv_igemm.hip:617)"),
    ("conv_ap.hip", ("conv3ap-stats1-acc1-fold0",),
     "STATS 1 comes from pcuda_conv2d_forward alone, which sets accumulate = 0 (conv_igemm.hip:617)"),
]
_UNREACHABLE_IDS = {i for _f, ids, _why in UNREACHABLE for i in ids}
REACHABLE = [i for i in INSTANTIATIONS if i not in _UNREACHABLE_IDS]

# plan branches: (name, predicate over (record, tag))
MECHANISMS = [
    ("conv3ap up1 forward", lambda r, t: t.startswith("conv3ap ") and " up1 " in t),
    ("conv3ap more items than compute units", lambda r, t: t.startswith("conv3ap ") and tag_int(t, "items") > 256),
    ("conv3ap one item", lambda r, t: t.startswith("conv3ap ") and tag_int(t, "items") == 1),
    ("conv3ap three co tiles", lambda r, t: t.startswith("conv3ap ") and tag_int(t, "rows") == 192),
    ("conv3ap two sources", lambda r, t: t.startswith("conv3ap ") and tag_int(t, "red") == 128 and "aff" in r["op"]),
    ("conv3ap split destination", lambda r, t: t.startswith("conv3ap ") and "split" in r["op"]),
    ("conv3rs h = 2", lambda r, t: t.startswith("conv3rs ") and " 2x32 " in t),
    ("conv3rs row segments", lambda r, t: t.startswith("conv3rs ") and " 37x32 " in t and tag_int(t, "items") == 2),
    ("conv3rs XCD mapping", lambda r, t: t.startswith("conv3rs ") and tag_int(t, "items") == 64),
    ("conv3rs three strips", lambda r, t: t.startswith("conv3rs ") and " 4x96 " in t),
] + [("wgrad3 %s ksplit %s" % (p, nm), (lambda r, t, p=p, f=f: t.startswith("wgrad3 ") and r["prec"] == p and f(tag_int(t, "ksplit"))))
     for p in BOTH for nm, f in (("1", lambda k: k == 1), ("2 .. 7", lambda k: 1 < k < 8), ("8 k", lambda k: k >= 8 and k % 8 == 0))] + [
    ("wgrad3r %s short last slice" % p, (lambda r, t, p=p: t.startswith("wgrad3r ") and r["prec"] == p and tag_int(t, "pairs") == 2 and tag_int(t, "slices") == 17))
    for p in BOTH] + [
    ("wgrad3r %s in_h 4" % p, (lambda r, t, p=p: t.startswith("wgrad3r ") and r["prec"] == p and " 4x32 " in t)) for p in BOTH] + [
    ("wgrad1 %s one step" % p, (lambda r, t, p=p: t.startswith("wgrad1 ") and r["prec"] == p and " steps1 " in t and " 4x4 " in t)) for p in BOTH] + [
    ("wgrad1 %s raised steps" % p, (lambda r, t, p=p: t.startswith("wgrad1 ") and r["prec"] == p and " steps15 " in t and " slices2 " in t)) for p in BOTH]


def _ratio(q):
    if q["e32"] > 0:
        return q["err"] / q["e32"]
    return 0.0 if q["err"] == 0 else float("inf")


@pytest.fixture(scope="module")
def sweep(dev, tmp_path_factory):
    """records of every operation of every table; a child that fails, is killed or runs into the hang guard fails the fixture
    (once: pytest caches the failure for the module, nothing is retried or started after it)"""
    tmp = tmp_path_factory.mktemp("special")
    records = []
    for table, switches in TABLES.items():
        out = str(tmp / (table + ".jsonl"))
        env = dict(os.environ, **switches)
        t0 = time.time()
        try:
            r = subprocess.run([sys.executable, CHILD, table, out], capture_output=True, text=True, timeout=CHILD_TIMEOUT, env=env)
        except subprocess.TimeoutExpired:
            pytest.fail("special child %r ran into the %d s hang guard" % (table, CHILD_TIMEOUT), pytrace=False)
        if r.returncode != 0:
            pytest.fail("special child %r exited with %s\n%s" % (table, r.returncode, r.stderr[-3000:]), pytrace=False)
        recs = [json.loads(ln) for ln in open(out)]
        assert recs and recs[-1].get("done"), "special child %r did not finish its table" % table
        print("child %s: %d operations, %.1f s wall, %.1f s of it in the sweep" % (table, len(recs) - 1, time.time() - t0, recs[-1]["seconds"]))
        records += recs[:-1]
    return records


def _describe(r):
    lines = ["%s [%s] %s %s -> %s" % (r["table"], r["case"], r["prec"], r["op"], r["last_kernel"])]
    for q in r["checks"]:
        lines.append("    %-12s err %.3e  e32 %.3e  ratio %6.2f (bound %.0f)   old %.3e (bound %.0e)" %
                     (q["what"], q["err"], q["e32"], _ratio(q), q["bound"] / q["e32"] if q["e32"] > 0 else 0.0, q["old_err"], q["old_bound"]))
    return "\n".join(lines)


def _assert_record(r):
    assert r["attributed"], "the intended kernel (%s) did not take the operation:\n%s" % (r["want"], _describe(r))
    assert r["fallbacks"] == 0, "fallback_count() moved:\n" + _describe(r)
    for q in r["checks"]:
        assert q["err"] <= q["bound"], "operand-exact bound (4 x chains x e32):\n" + _describe(r)
        assert q["old_err"] < q["old_bound"], "the project's bound:\n" + _describe(r)


@pytest.mark.parametrize("inst", REACHABLE)
def test_instantiation(sweep, inst):
    mine = [r for r in sweep if inst_of(r["last_kernel"], r["prec"]) == inst]
    assert mine, "no operation of the sweep ran %s" % inst
    for r in mine:
        print(_describe(r))
    for r in mine:
        _assert_record(r)


def test_every_operation_attributed_and_within_bounds(sweep):
    worst = {}
    for r in sweep:
        print(_describe(r))
        fam = (inst_of(r["last_kernel"], r["prec"]) or "?").split("-")[0] + " " + r["prec"]
        for q in r["checks"]:
            worst[fam] = max(worst.get(fam, 0.0), _ratio(q))
    print("largest kernel error / e32 per kernel and precision:", {k: round(v, 3) for k, v in sorted(worst.items())})
    assert len(sweep) > 200
    for r in sweep:
        _assert_record(r)


def test_every_listed_instantiation_ran(sweep):
    seen = {inst_of(r["last_kernel"], r["prec"]) for r in sweep if r["attributed"]}
    assert len(INSTANTIATIONS) == len(set(INSTANTIATIONS)) == 12 + 8 + 4 + 2 + 12 + 18
    files = [f for f, _ids, _why in UNREACHABLE]
    assert len(files) == len(set(files))
    for _f, ids, why in UNREACHABLE:
        assert why and all(i in INSTANTIATIONS for i in ids)
        stale = [i for i in ids if i in seen]
        assert not stale, "listed as unreachable but launched: %s" % stale
    missing = [i for i in REACHABLE if i not in seen]
    assert not missing, missing
    # every launch of the sweep is one of the listed instantiations (a tag this file cannot place is an error of the list)
    assert None not in {inst_of(r["last_kernel"], r["prec"]) for r in sweep}
    assert seen <= set(INSTANTIATIONS), seen - set(INSTANTIATIONS)
    for name, pred in MECHANISMS:
        assert any(r["attributed"] and pred(r, r["last_kernel"]) for r in sweep), "no operation reached: " + name
