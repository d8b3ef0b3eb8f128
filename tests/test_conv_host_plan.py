"""The host-side decisions of the 2-D convolution dispatch, pinned against tests/golden/conv_host_plan.json (recorded by
scripts/make_conv_host_golden.py on the parent of the host-dispatch refactor): packed buffer sizes, tile counts and the job
records of the batched repack for every geometry of the script's list, both precisions, with and without the small-map
knobs.  Pure host code: no device is needed (the compute-unit count then falls back to 256, the MI355X's own)."""
import importlib.util
import json
import os

from conftest import GOLD, ROOT

_spec = importlib.util.spec_from_file_location("make_conv_host_golden", os.path.join(ROOT, "scripts", "make_conv_host_golden.py"))
gen = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(gen)


def test_host_plan_matches_the_recorded_one():
    from pointcloududa_amd import _lib
    with open(os.path.join(GOLD, "conv_host_plan.json")) as fh:
        want = json.load(fh)
    assert want["geoms"] == [list(t) for t in gen.GEOMS] and len(want["geoms"]) >= 60, "fixture and geometry list disagree"
    assert want["job_fields"] == list(gen.JOB_FIELDS)
    got = gen.record(_lib.lib())
    assert sorted(got) == sorted(want["records"]) and len(got) == 4
    diffs = []
    for key in sorted(got):
        assert len(got[key]) == len(want["records"][key]) == len(gen.GEOMS)
        for t, a, b in zip(gen.GEOMS, got[key], want["records"][key]):
            for f in b:
                if a[f] != b[f]:
                    diffs.append((key, t, f, a[f], b[f]))
    assert not diffs, "%d differences, the first: %r" % (len(diffs), diffs[:3])


def test_fixture_reaches_every_branch():
    """the recorded list is only a pin if the branches it names are taken in it"""
    with open(os.path.join(GOLD, "conv_host_plan.json")) as fh:
        want = json.load(fh)
    fields = want["job_fields"]
    rec, pair = fields.index("rec"), fields.index("pair")
    jobs = [j for r in want["records"]["default/prec0"] for j in r["jobs_all"]["jobs"]]
    assert any(j[rec] == 32 for j in jobs) and any(j[pair] == 1 for j in jobs) and any(j[rec] == 72 for j in jobs)
    assert any(j[rec] == 40 for r in want["records"]["default/prec1"] for j in r["jobs_all"]["jobs"])
    assert any(r["jobs_all"]["n"] == 10 for r in want["records"]["default/prec0"])          # stride 3: nine classes
    assert any(r["jobs_all"]["n"] < 0 and r["fwd_bytes"] == 0 for r in want["records"]["default/prec0"])   # refused geometry
    a, b = want["records"]["default/prec0"], want["records"]["small_maps/prec0"]
    assert any(x["fwd_tiles"] != y["fwd_tiles"] for x, y in zip(a, b)), "the knobs change no route in this list"
    assert all(x["jobs_all"] == y["jobs_all"] and x["fwd_bytes"] == y["fwd_bytes"] for x, y in zip(a, b)), \
        "a packed buffer must not depend on the map knobs"
