"""The BatchNorm / LeakyReLU / pooling / point-max family on the device (csrc/pointwise.hip, csrc/pointnet_small.hip and
their wrappers in kernels.py), pinned against the records of tests/golden/pointwise_pin.json
(scripts/make_pointwise_pin_golden.py, recorded on the parent of the refactor that gave the family one statement of its
arithmetic, csrc/bn_device.h): per case the launches of every call and the sha256 of every output tensor and of the inputs
(one digest over a case's named tensor hashes each: a case differs as soon as one tensor does).
The kernels sum in a fixed order and the library is compiled without contraction, so the hashes repeat bit for bit: there is
no tolerance.  Where the recorded toolchain is not the running one, the failure says so."""
import os
import sys

import pytest

from conftest import GOLD, ROOT

pytestmark = pytest.mark.gpu

sys.path.insert(0, os.path.join(ROOT, "scripts"))
import make_pointwise_pin_golden as gen  # noqa: E402
import pin_common as P  # noqa: E402


@pytest.fixture(scope="module")
def records(dev):
    return gen.record(dev)


@pytest.fixture(scope="module")
def golden():
    return P.load_golden(os.path.join(GOLD, "pointwise_pin.json"))


def test_the_case_list_is_the_recorded_one(records, golden):
    P.assert_case_list(records, golden)


def test_every_output_bit_and_launch_count_matches(records, golden):
    P.assert_no_differences(records, golden)
