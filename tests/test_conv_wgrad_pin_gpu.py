"""The weight-gradient routes on the device, pinned against the records of tests/golden/conv_wgrad_plan.json
(scripts/make_conv_wgrad_golden.py, recorded on the parent of the route-table refactor): per case, precision, bias gradient
and accumulate flag the launch tag, the ``fallback_count()`` delta, the reduce job of ``pcuda_conv2d_wgrad_partial`` and the
sha256 of dw and db -- from ``pcuda_conv2d_wgrad`` and from partial + ``pcuda_wgrad_reduce_batch``, which must also agree
with each other.  Inputs are multiples of 2^-8 and the kernels sum in a fixed order, so the hashes repeat bit for bit.

The cases run in child processes (tests/conv_wgrad_child.py, one per table of route switches, one after the other, each
under its own timeout; nothing is started after a child that fails)."""
import importlib.util
import json
import os

import pytest

from conftest import GOLD, ROOT

pytestmark = pytest.mark.gpu

_spec = importlib.util.spec_from_file_location("make_conv_wgrad_golden", os.path.join(ROOT, "scripts", "make_conv_wgrad_golden.py"))
gen = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(gen)


@pytest.fixture(scope="module")
def records(dev, tmp_path_factory):
    try:
        return gen.record_device(str(tmp_path_factory.mktemp("wgrad_pin")))
    except Exception as e:      # a child failed, was killed or ran into the hang guard: once, nothing is retried
        pytest.fail("weight-gradient pin: %s" % e, pytrace=False)


def test_records_match_the_recorded_ones(records):
    with open(os.path.join(GOLD, "conv_wgrad_plan.json")) as fh:
        want = json.load(fh)["device"]
    key = lambda r: (r["table"], r["case"], r["prec"], r["db"], r["acc"])
    assert [key(r) for r in records] == [key(r) for r in want], "fixture and case list disagree"
    diffs = [(key(a), f, a[f], b[f]) for a, b in zip(records, want) for f in b if a[f] != b[f]]
    assert not diffs, "%d differences, the first: %r" % (len(diffs), diffs[:3])


def test_batched_reduce_equals_the_one_by_one_reduce(records):
    for r in records:
        assert r["hash"]["dw"] == r["hash"]["dw_batch"] and r["hash"]["db"] == r["hash"]["db_batch"], r


def test_every_branch_is_reached(records):
    assert not gen.child.missing_branches(records)
