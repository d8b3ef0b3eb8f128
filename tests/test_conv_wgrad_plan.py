"""The weight-gradient host side, pinned against tests/golden/conv_wgrad_plan.json (recorded by
scripts/make_conv_wgrad_golden.py on the parent of the route-table refactor): ``pcuda_conv2d_wgrad_workspace_size`` for every
geometry of the script's list under four sets of the route switches, each set in a child process of its own (the switches are
cached per process).  Pure host code: nothing is launched and no device is needed.  The fixture's device records are compared
by tests/test_conv_wgrad_pin_gpu.py; that they reach the branches they were recorded for is checked here."""
import importlib.util
import json
import os

from conftest import GOLD, ROOT

_spec = importlib.util.spec_from_file_location("make_conv_wgrad_golden", os.path.join(ROOT, "scripts", "make_conv_wgrad_golden.py"))
gen = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(gen)


def _fixture():
    with open(os.path.join(GOLD, "conv_wgrad_plan.json")) as fh:
        return json.load(fh)


def test_workspace_sizes_match_the_recorded_ones():
    want = _fixture()
    geoms = gen.host_geoms()
    assert want["host_geoms"] == [list(t) for t in geoms] and len(geoms) >= 80, "fixture and geometry list disagree"
    got = gen.record_host()
    assert sorted(got) == sorted(want["host"]) == sorted(gen.HOST_KNOBS) and len(got) == 4
    diffs = [(k, t, a, b) for k in sorted(got) for t, a, b in zip(geoms, got[k], want["host"][k]) if a != b]
    assert not diffs, "%d differences, the first: %r" % (len(diffs), diffs[:3])


def test_fixture_reaches_every_branch():
    """the recorded list is only a pin if the switches and the branches it names show in it"""
    want = _fixture()
    gen.check_host(want["host"])          # every two knob sets differ on some geometry
    host = dict(zip(map(tuple, want["host_geoms"]), want["host"]["default"]))
    assert host[tuple(gen.SLAB_CAP)] == gen.geom_slab_bytes(gen.SLAB_CAP, 4), "the 64 MB cap: 8 slices of 9.4 MB halved to 4"
    assert host[(0,) * 10] == 0           # refused geometry
    assert len(want["device"]) > 300
    assert not gen.child.missing_branches(want["device"])
    for r in want["device"]:
        assert r["hash"]["dw"] == r["hash"]["dw_batch"] and r["hash"]["db"] == r["hash"]["db_batch"], r
