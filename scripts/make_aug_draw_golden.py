"""Writes tests/golden/aug_draw_digests.json: what every sampler of the augmentation layer (pointcloududa_amd/utils; DESIGN.md
section 6) draws from a seeded generator, and how much of the generator it consumes.

Per call the sha256 over every array the sampler returns (name, dtype, shape, bytes; a ``HeavyPlan``'s stages in order, each
with its type name) and the next ``rng.integers(0, 2**62)`` after the call, for the seeds 0..9 at ``B, H, W = 16, 64, 48`` and
``6, 40, 41``:

* every heavy preset through ``sample_heavy_plan``, ``sample_geo_program`` and ``sample_style_program`` (``"ValueError"`` where a
  preset holds no stylize entry)
* ``sample_program(B, "mscmrseg_aug2_photometric", rng)``
* ``sample_params(B, preset, rng)`` for both light presets

The file is recorded on a commit whose draws are to be kept (tests/test_aug_draws_pinned.py recomputes and compares): a change of
the samplers' code must leave it as it is.

    python scripts/make_aug_draw_golden.py            # writes the file
    python scripts/make_aug_draw_golden.py --check    # recomputes and compares with the file"""
import hashlib
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PATH = os.path.join(ROOT, "tests", "golden", "aug_draw_digests.json")
SHAPES = ((16, 64, 48), (6, 40, 41))
SEEDS = 10
PHOTO_PRESET = "mscmrseg_aug2_photometric"
LIGHT_PRESETS = ("mmwhs_light", "mscmrseg_simple")


def _update(h, obj):
    for name in sorted(vars(obj)):
        a = np.ascontiguousarray(getattr(obj, name))
        h.update(("%s|%s|%r|" % (name, a.dtype.str, a.shape)).encode())
        h.update(a.tobytes())


def digest(obj):
    """sha256 of a program / parameter object (every field of ``vars``: name, dtype, shape, bytes) or of a plan (``batch``, then
    each stage's type name and fields)"""
    h = hashlib.sha256()
    if hasattr(obj, "stages"):
        h.update(("batch|%d|" % obj.batch).encode())
        for st in obj.stages:
            h.update(type(st).__name__.encode())
            _update(h, st)
    else:
        _update(h, obj)
    return h.hexdigest()


def calls():
    """-> [(key, f(rng))]: every pinned call"""
    sys.path.insert(0, ROOT)
    from pointcloududa_amd.utils import augment as A
    from pointcloududa_amd.utils.heavy import _PRESETS
    out = []
    for b, h, w in SHAPES:
        tag = "%dx%dx%d" % (b, h, w)
        for preset in sorted(_PRESETS):
            for fn in (A.sample_heavy_plan, A.sample_geo_program, A.sample_style_program):
                out.append(("%s|%s|%s" % (fn.__name__, preset, tag), lambda rng, fn=fn, p=preset, b=b, h=h, w=w: fn(b, p, rng, h, w)))
        out.append(("sample_program|%s|%s" % (PHOTO_PRESET, tag), lambda rng, b=b: A.sample_program(b, PHOTO_PRESET, rng)))
        for preset in LIGHT_PRESETS:
            out.append(("sample_params|%s|%s" % (preset, tag), lambda rng, p=preset, b=b: A.sample_params(b, p, rng)))
    return out


def build():
    """-> {key: [[digest or "ValueError", next draw] per seed]}"""
    rec = {}
    for key, f in calls():
        rows = []
        for seed in range(SEEDS):
            rng = np.random.default_rng(seed)
            try:
                d = digest(f(rng))
            except ValueError:
                d = "ValueError"
            rows.append([d, int(rng.integers(0, 2 ** 62))])
        rec[key] = rows
    return rec


if __name__ == "__main__":
    new = build()
    if "--check" in sys.argv:
        old = json.load(open(PATH))
        bad = sorted(k for k in set(old) | set(new) if old.get(k) != new.get(k))
        if bad:
            raise SystemExit("differs from %s: %s" % (PATH, ", ".join(bad)))
        print("equal:", PATH, len(new), "calls")
    else:
        with open(PATH, "w") as f:
            json.dump(new, f, indent=0, sort_keys=True)
            f.write("\n")
        print("wrote", PATH, os.path.getsize(PATH), "bytes")
