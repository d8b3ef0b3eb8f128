"""Every loss entry point on the device, pinned against the records of tests/golden/loss_pin.json
(scripts/make_loss_pin_golden.py, recorded on the parent of the overlap-loss refactor): per case the launches of the forward
and of every backward call and the sha256 of every output tensor -- scalars, gradients, maps, the bad-label counter.  The
kernels sum in a fixed order, the library is compiled without contraction: the hashes repeat bit for bit, and there is no
tolerance anywhere.  The hashes depend on the toolchain as well as on the sources: where the recorded one is not the running
one, the failure says so.  (The comparison itself is scripts/pin_common.py's, shared with the pointwise pin.)"""
import os
import sys

import pytest

from conftest import GOLD, ROOT

pytestmark = pytest.mark.gpu

sys.path.insert(0, os.path.join(ROOT, "scripts"))
import make_loss_pin_golden as gen  # noqa: E402
import pin_common as P  # noqa: E402


@pytest.fixture(scope="module")
def records(dev):
    return gen.record(dev)


@pytest.fixture(scope="module")
def golden():
    return P.load_golden(os.path.join(GOLD, "loss_pin.json"))


def test_the_case_list_is_the_recorded_one(records, golden):
    P.assert_case_list(records, golden)


def test_every_output_bit_and_launch_count_matches(records, golden):
    P.assert_no_differences(records, golden)
