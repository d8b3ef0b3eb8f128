"""Every template instantiation of the default build's convolution kernels (csrc/built_variants.h: 44 pipe + 31 ig8 + 52
wgrad keys) against the operand-exact reference of tests/conv_exact_ref.py, attributed key by key.

``PCUDA_VARIANT_LOG`` and the library's A/B switches are read once per process, so the sweep runs in child processes
(tests/conv_variant_child.py, one per case table, one after the other: parent + one child hold the GPU at a time), each with a
fresh log; the child re-reads the log after every operation, so every key belongs to the operation that dispatched it first.
Per key: that operation exists, and all it computed is within BOTH bounds -- 4 x chains x e32 per output channel against
the operand-exact float64 reference (e32 = the same expression in float32 on the CPU, computed per case from the reference
alone; chains = 1 in bf16 mode, 3 in bf16x3 mode, below) -- and the project's 1e-4 / 2e-2 of the tensor's scale against the
unrounded float64 convolution.

Tables: ``pipe``, ``ig8``, ``wgrad`` with the default dispatcher, and ``wgrad_no_wgrad1`` (PCUDA_NO_WGRAD1=1): the 1x1 /
stride-1 kernel of csrc/conv_wgrad1.hip (wgrad1_wgrad, in front of the generic plan in WGRAD_ROUTES, csrc/conv_wgrad.hip:336)
takes every 1x1 shape with whole 32-channel chunks and rows of 16k pixels, which is what keys 576-579 (mode 0, one tap, quad
staging) need too: with cin >= 32 they run only behind that switch.  The anti-phase, row-streaming, wgrad3 and direct kernels
pre-empt no built key at EVERY shape: the other 123 keys are reached with the default dispatcher.

UNREACHABLE is empty: the search (the child's docstring) found a geometry of at most 1.1e9 multiply-adds for all 127 keys.

Measured on an MI355X, largest kernel error / e32 over every check of every operation (the kernels are deterministic: the
figures repeat run to run):
    family   bf16 (bound 4)   bf16x3 (bound 12)
    pipe     2.58             7.56   (convolution outputs 6.39: forward 512 -> 32, 2x2 stride 2, 2048 products per output;
                                      7.56 / 7.01 / 6.18: the BatchNorm-backward partial sums over 75 264 gradients per channel)
    ig8      2.90             3.92
    wgrad    1.48             2.57
The finding behind ``chains``: with the factor 4 alone every bf16 check passed and six bf16x3 checks of the ``pipe`` table did
not (the figures above).  Cause, from the MFMA phases: a bf16x3 kernel adds its three product planes into ONE accumulator, three
roundings per 16-product step at the magnitude of the running full sum, where the float32 evaluation behind e32 convolves each
plane on its own -- one chain (tests/conv_exact_ref.py, ACC_CHAINS).  The bound follows the number of chains, a property of the
reference's expression and of the kernel's source, not of what the kernels returned; torch's float32 ``sum`` behind the partial
sums' e32 is pairwise, the tightest of the correct orders.

Self-check (scratch copy, not committed): scaling channel 31 of every chunk by 0.999 in the PF = 3 / XQ / mode 1 / 9-tap /
64-row instantiation of ``wgrad_kernel`` fails exactly wgrad-662, wgrad-663 and the all-operations test (error 1.0e-3 against
bounds of 8e-7 / 2.7e-6) while the bf16 case stays inside the old 2e-2 (3.4e-3).

Wall time of the four children on that machine: 17 s together (pipe 10 s, of which 7.8 s in the sweep -- the float64
references of its 19 cases; the others 2-3 s each, almost all of it starting Python and loading the library; the GPU work of
a case is milliseconds).  CHILD_TIMEOUT is a hang guard of more than ten times the slowest child.
"""
import json
import os
import subprocess
import sys
import time

import pytest

import conv_exact_ref as R
from conv_variant_child import TABLES

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
CHILD = os.path.join(HERE, "conv_variant_child.py")
LISTS, _COUNTS = R.parse_built_variants()

# Keys no geometry within the size limit dispatches: (family, key, dispatcher condition or pre-empting kernel).  At most one
# key in ten per family; a key listed here must not appear in any child's log (test_unreachable_list_is_not_stale).
UNREACHABLE = []
MAX_UNREACHABLE = {"pipe": 4, "ig8": 3, "wgrad": 5}

CHILD_TIMEOUT = 600    # seconds; a hang guard, not a budget

KEYS = [(f, k) for f in ("pipe", "ig8", "wgrad") for k in LISTS[f] if (f, k) not in {(u[0], u[1]) for u in UNREACHABLE}]


def _ratio(q):
    if q["e32"] > 0:
        return q["err"] / q["e32"]
    return 0.0 if q["err"] == 0 else float("inf")


@pytest.fixture(scope="module")
def sweep(dev, tmp_path_factory):
    """records of every operation of every table, and each child's log; a child that fails, is killed or runs into the hang
    guard fails the fixture (once: pytest caches the failure for the module, nothing is retried or started after it)"""
    tmp = tmp_path_factory.mktemp("variants")
    records, logs = [], {}
    for table, (_kind, switches, _cases) in TABLES.items():
        log, out = str(tmp / (table + ".log")), str(tmp / (table + ".jsonl"))
        env = dict(os.environ, PCUDA_VARIANT_LOG=log, **switches)
        t0 = time.time()
        try:
            r = subprocess.run([sys.executable, CHILD, table, out], capture_output=True, text=True, timeout=CHILD_TIMEOUT, env=env)
        except subprocess.TimeoutExpired:
            pytest.fail("variant child %r ran into the %d s hang guard" % (table, CHILD_TIMEOUT), pytrace=False)
        if r.returncode != 0:
            pytest.fail("variant child %r exited with %s\n%s" % (table, r.returncode, r.stderr[-3000:]), pytrace=False)
        recs = [json.loads(ln) for ln in open(out)]
        assert recs and recs[-1].get("done"), "variant child %r did not finish its table" % table
        print("child %s: %d operations, %.1f s wall, %.1f s of it in the sweep" % (table, len(recs) - 1, time.time() - t0, recs[-1]["seconds"]))
        records += recs[:-1]
        with open(log) as fh:
            logs[table] = {(ln.split()[0], int(ln.split()[1])) for ln in fh if ln.strip()}
    return records, logs


def _describe(r):
    lines = ["%s %s %s %s -> %s" % (r["table"], tuple(r["case"]), r["prec"], r["op"], r["last_kernel"])]
    for q in r["checks"]:
        lines.append("    %-12s err %.3e  e32 %.3e  ratio %6.2f (bound %.0f)   old %.3e (bound %.0e)" %
                     (q["what"], q["err"], q["e32"], _ratio(q), q["bound"] / q["e32"] if q["e32"] > 0 else 0.0, q["old_err"], q["old_bound"]))
    return "\n".join(lines)


def _assert_within(r):
    for q in r["checks"]:
        assert q["err"] <= q["bound"], "operand-exact bound (4 x chains x e32):\n" + _describe(r)
        assert q["old_err"] < q["old_bound"], "the project's bound:\n" + _describe(r)


@pytest.mark.parametrize("family,key", KEYS, ids=[R.variant_id(f, k) for f, k in KEYS])
def test_built_variant(sweep, family, key):
    records, _ = sweep
    first = [r for r in records if [family, key] in r["keys"]]
    assert first, "no operation of the sweep dispatched %s (fields %s)" % (R.variant_id(family, key), R.FIELDS_FN[family](key))
    x3 = R.FIELDS_FN[family](key)["x3"]
    for r in first:
        print(_describe(r))
        assert r["prec"] == ("bf16x3" if x3 else "bf16"), r
        _assert_within(r)


def test_every_operation_within_bounds(sweep):
    records, _ = sweep
    worst = {}
    for r in records:
        print(_describe(r))
        fam = r["table"].split("_")[0]
        for q in r["checks"]:
            worst[fam] = max(worst.get(fam, 0.0), _ratio(q))
    print("largest kernel error / e32 per table family:", {k: round(v, 3) for k, v in worst.items()})
    assert len(records) > 400
    for r in records:
        _assert_within(r)


def test_unreachable_list_is_not_stale(sweep):
    _, logs = sweep
    seen = set().union(*logs.values())
    for fam, cap in MAX_UNREACHABLE.items():
        assert sum(1 for u in UNREACHABLE if u[0] == fam) <= cap, fam
    for fam, key, why in UNREACHABLE:
        assert key in LISTS[fam] and why
        assert (fam, key) not in seen, "%s is listed as unreachable but was dispatched" % R.variant_id(fam, key)
    # and the other way round: everything built and not listed was dispatched by some child
    missing = [R.variant_id(f, k) for f, k in KEYS if (f, k) not in seen]
    assert not missing, missing
