"""The samplers of the augmentation layer draw what they drew and consume the generator as they did: every heavy preset through
``sample_heavy_plan`` / ``sample_geo_program`` / ``sample_style_program``, the photometric preset and both light presets, seeds
0..9 at two batch shapes, against tests/golden/aug_draw_digests.json (scripts/make_aug_draw_golden.py: recorded on the commit
before the layer was reorganised around ``utils/_program.py`` and ``utils/heavy.py``)."""
import importlib.util
import json
import os

from conftest import GOLD, ROOT


def _load(name):
    spec = importlib.util.spec_from_file_location(name, os.path.join(ROOT, "scripts", name + ".py"))
    m = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(m)
    return m


def test_every_sampler_draws_and_consumes_what_it_did():
    G = _load("make_aug_draw_golden")
    from pointcloududa_amd.utils import heavy
    want = json.load(open(os.path.join(GOLD, "aug_draw_digests.json")))
    assert os.path.getsize(os.path.join(GOLD, "aug_draw_digests.json")) < 100000
    got = G.build()
    assert sorted(got) == sorted(want) and len(want) == len(G.SHAPES) * (3 * len(heavy._PRESETS) + 1 + len(G.LIGHT_PRESETS))
    assert len(heavy._PRESETS) == 8 and G.SHAPES == ((16, 64, 48), (6, 40, 41)) and G.SEEDS == 10
    for key in sorted(want):
        assert len(want[key]) == G.SEEDS
        for seed, (a, b) in enumerate(zip(got[key], want[key])):
            assert a[0] == b[0], "%s, seed %d: the drawn arrays differ" % (key, seed)
            assert a[1] == b[1], "%s, seed %d: the generator is consumed differently" % (key, seed)
    # a preset without a stylize entry raises in sample_style_program, and only there
    refused = {k for k, rows in want.items() if any(r[0] == "ValueError" for r in rows)}
    assert refused == {"sample_style_program|%s|%dx%dx%d" % ((p,) + s) for p in ("heavy_device", "mscmrseg_aug2_device")
                       for s in G.SHAPES}
    assert all(r[0] == "ValueError" for k in refused for r in want[k])
