"""Every loss entry point on the device, pinned against the records of tests/golden/loss_pin.json
(scripts/make_loss_pin_golden.py, recorded on the parent of the overlap-loss refactor): per case the launches of the forward
and of every backward call and the sha256 of every output tensor -- scalars, gradients, maps, the bad-label counter.  The
kernels sum in a fixed order, the library is compiled without contraction: the hashes repeat bit for bit, and there is no
tolerance anywhere.  The hashes depend on the toolchain as well as on the sources: where the recorded one is not the running
one, the failure says so."""
import importlib.util
import json
import os

import pytest

from conftest import GOLD, ROOT

pytestmark = pytest.mark.gpu

_spec = importlib.util.spec_from_file_location("make_loss_pin_golden", os.path.join(ROOT, "scripts", "make_loss_pin_golden.py"))
gen = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(gen)


@pytest.fixture(scope="module")
def records(dev):
    return gen.record(dev)


@pytest.fixture(scope="module")
def golden():
    with open(os.path.join(GOLD, "loss_pin.json")) as fh:
        return json.load(fh)


def _toolchains(golden):
    now = gen.toolchain()
    if now == golden["toolchain"]:
        return "same toolchain as recorded (%r)" % (now,)
    return "the toolchain differs: recorded %r, running %r" % (golden["toolchain"], now)


def test_the_case_list_is_the_recorded_one(records, golden):
    assert [r["case"] for r in records] == [r["case"] for r in golden["records"]], "fixture and case list disagree"


def test_every_output_bit_and_launch_count_matches(records, golden):
    want = {r["case"]: r for r in golden["records"]}
    diffs = []
    for r in records:
        w = want[r["case"]]
        for field in ("in", "launches", "hash"):
            assert sorted(r[field]) == sorted(w[field]), (r["case"], field)
            diffs += [(r["case"], field, k, r[field][k], w[field][k]) for k in w[field] if r[field][k] != w[field][k]]
    assert not diffs, "%d differences (%s), the first: %r" % (len(diffs), _toolchains(golden), diffs[:3])
