"""The recipes of the heavy pipelines on the device: which entries of the four operator
families (``photometric``, ``geometric``, ``stylize``, ``croppad``) a preset holds, how one batch selects and orders them
(``_select``), the plan that interleaves them (``sample_heavy_plan``, ``HeavyPlan``, ``heavy_aug``) and the geometric / stylize
entries of a preset alone (``sample_geo_program``, ``sample_style_program``).  The operator modules know nothing of presets.

``interp`` (f8b), a keyword of the three samplers: ``"linear"`` (the default) draws what has always been drawn.  ``"cubic"``
encodes every ElasticTransformation slot with order 3 (imgaug's default for it; no extra draw) and, AFTER every other draw
of the call, draws one more ``rng.random(B)``: the SimplexNoiseAlpha slot of sample ``i`` takes ``UPSCALE_CUBIC`` where that value
is below ``stylize.NOISE_CUBIC_P`` (0.35, this build's choice: recalled as imgaug's default weight, not checkable here).  Every
other array equals the linear draw of the same generator state.  No preset is added."""
from __future__ import annotations

from dataclasses import dataclass, field
from typing import List, Optional, Union

import numpy as np
import torch

from . import stylize as St
from ._program import HEAVY_MESSAGE
from .croppad import CropPadProgram
from .geometric import (ENTRY_AFFINE, ENTRY_CROP_AND_PAD, ENTRY_ELASTIC, ENTRY_FLIPLR, ENTRY_FLIPUD, ENTRY_PERSPECTIVE,
                        ENTRY_PIECEWISE, FLIP_LR_P, FLIP_UD_P, SOMEOF_COUNT, SOMETIMES_P, GeoProgram, _draw_geo, _encode_geo,
                        crop_pad_pixels)
from .photometric import PhotoProgram, draw_photo, encode_photo
from .stylize import StyleProgram

HEAVY_DEVICE_PRESET, AUG2_DEVICE_PRESET = "heavy_device", "mscmrseg_aug2_device"
HEAVY_FULL_PRESET, AUG2_FULL_PRESET = "heavy_full_device", "mscmrseg_aug2_full_device"
HEAVY_REFPAD_PRESET, AUG2_REFPAD_PRESET = "heavy_refpad_device", "mscmrseg_aug2_refpad_device"
HEAVY_CONNECTED_PRESET, AUG2_CONNECTED_PRESET = "heavy_connected_device", "mscmrseg_aug2_connected_device"
HEAVY_SCALED_PRESET, AUG2_SCALED_PRESET = "heavy_scaled_device", "mscmrseg_aug2_scaled_device"

_PHOTO_BLOCK = tuple(("p", e) for e in range(9))
# the reference's list order: Superpixels, blur, sharpen, emboss, SimplexNoiseAlpha, noise, dropout, invert, add, hue, ...
_FULL_BLOCK = ((("s", St.ENTRY_SUPERPIXELS),) + _PHOTO_BLOCK[:3] + (("s", St.ENTRY_NOISE_ALPHA),) + _PHOTO_BLOCK[3:7] +
               (("s", St.ENTRY_HUE),) + _PHOTO_BLOCK[7:])
_PRESETS = {
    # data_generator_mscmrseg.py:23-82 minus Superpixels, SimplexNoiseAlpha, AddToHueAndSaturation
    HEAVY_DEVICE_PRESET: dict(
        outer=(("g", ENTRY_FLIPLR), ("g", ENTRY_FLIPUD), ("g", ENTRY_CROP_AND_PAD), ("g", ENTRY_AFFINE), "block"),
        block=_PHOTO_BLOCK + (("g", ENTRY_ELASTIC), ("g", ENTRY_PIECEWISE), ("g", ENTRY_PERSPECTIVE))),
    # data_generator_mscmrseg.py:89-130 minus the same three
    AUG2_DEVICE_PRESET: dict(outer=(("g", ENTRY_CROP_AND_PAD), "block"), block=_PHOTO_BLOCK),
    # data_generator_mscmrseg.py:23-82, all fifteen SomeOf entries (f9)
    HEAVY_FULL_PRESET: dict(
        outer=(("g", ENTRY_FLIPLR), ("g", ENTRY_FLIPUD), ("g", ENTRY_CROP_AND_PAD), ("g", ENTRY_AFFINE), "block"),
        block=_FULL_BLOCK + (("g", ENTRY_ELASTIC), ("g", ENTRY_PIECEWISE), ("g", ENTRY_PERSPECTIVE))),
    # data_generator_mscmrseg.py:89-130, all twelve
    AUG2_FULL_PRESET: dict(outer=(("g", ENTRY_CROP_AND_PAD), "block"), block=_FULL_BLOCK),
    # the two full recipes with CropAndPad over all ten modes of numpy.pad, a CropPadProgram stage of its own (f14)
    HEAVY_REFPAD_PRESET: dict(
        outer=(("g", ENTRY_FLIPLR), ("g", ENTRY_FLIPUD), ("c", ENTRY_CROP_AND_PAD), ("g", ENTRY_AFFINE), "block"),
        block=_FULL_BLOCK + (("g", ENTRY_ELASTIC), ("g", ENTRY_PIECEWISE), ("g", ENTRY_PERSPECTIVE))),
    AUG2_REFPAD_PRESET: dict(outer=(("c", ENTRY_CROP_AND_PAD), "block"), block=_FULL_BLOCK),
}
# the two _refpad_ recipes, draw for draw, with connected superpixels: min_size = superpixel_min_size(..) on every Superpixels
# slot (f9b)
_PRESETS[HEAVY_CONNECTED_PRESET] = dict(_PRESETS[HEAVY_REFPAD_PRESET], connected=True)
_PRESETS[AUG2_CONNECTED_PRESET] = dict(_PRESETS[AUG2_REFPAD_PRESET], connected=True)
# the two _connected_ recipes, draw for draw, with imgaug's max_size = 128 on every Superpixels slot: the grid and min_size
# are those of the working size (f9c).  A table of its own: tests/golden/aug_draw_digests.json records the draws of every
# preset of _PRESETS, while these two are pinned by their relation to their _connected_ twins (tests/test_spx_scaled.py)
_SCALED_PRESETS = {HEAVY_SCALED_PRESET: dict(_PRESETS[HEAVY_CONNECTED_PRESET], scaled=True),
                   AUG2_SCALED_PRESET: dict(_PRESETS[AUG2_CONNECTED_PRESET], scaled=True)}
_SOMETIMES = {("g", ENTRY_ELASTIC), ("g", ENTRY_PIECEWISE), ("g", ENTRY_PERSPECTIVE), ("s", St.ENTRY_SUPERPIXELS)}
_OUTER_P = {ENTRY_FLIPLR: FLIP_LR_P, ENTRY_FLIPUD: FLIP_UD_P, ENTRY_CROP_AND_PAD: SOMETIMES_P, ENTRY_AFFINE: SOMETIMES_P}
_STAGE_TYPES = {"p": PhotoProgram, "g": GeoProgram, "s": StyleProgram, "c": CropPadProgram}


def _check_preset(preset):
    if preset == "heavy":
        raise NotImplementedError(HEAVY_MESSAGE)
    if preset in _SCALED_PRESETS:
        return _SCALED_PRESETS[preset]
    if preset not in _PRESETS:
        raise ValueError("unknown heavy preset %r (have: %s)" % (preset, ", ".join(sorted(set(_PRESETS) | set(_SCALED_PRESETS)))))
    return _PRESETS[preset]


def _select(b, spec, rng):
    """-> (entries in application order, on bool [B, len(entries)]): one outer and one inner order per batch
    (``random_order=True`` as f6 and f7 draw it); ``SomeOf((0, 5))`` picks a uniform count of distinct block entries per
    sample, and the three warps inside the block (and, in the full presets, Superpixels) sit behind ``sometimes(0.5)``"""
    outer, block = spec["outer"], spec["block"]
    outer_order, inner_order = rng.permutation(len(outer)), rng.permutation(len(block))
    count = rng.integers(SOMEOF_COUNT[0], SOMEOF_COUNT[1] + 1, b)
    rank = np.argsort(np.argsort(rng.random((b, len(block))), axis=1), axis=1)
    chosen = rank < count[:, None]
    for k, entry in enumerate(block):
        if entry in _SOMETIMES:
            chosen[:, k] &= rng.random(b) < SOMETIMES_P
    outer_on = {k: rng.random(b) < _OUTER_P[e[1]] for k, e in enumerate(outer) if e != "block"}
    entries, on = [], []
    for k in outer_order:
        if outer[k] == "block":
            for q in inner_order:
                entries.append(block[q])
                on.append(chosen[:, q])
        else:
            entries.append(outer[k])
            on.append(outer_on[k])
    return entries, np.stack(on, axis=1)


INTERPS = ("linear", "cubic")


def _check_interp(interp):
    if interp not in INTERPS:
        raise ValueError("unknown interp %r (have: %s)" % (interp, ", ".join(INTERPS)))
    return interp == "cubic"


def _cubic_upscale(prog, cubic_draw):
    """the noise-alpha slots of the samples whose draw fell below NOISE_CUBIC_P upscale cubically"""
    pick = (prog.opcode == St.OP_NOISE_ALPHA_CONV3X3) & (cubic_draw < St.NOISE_CUBIC_P)[:, None]
    prog.iarg[..., 1][pick] = St.UPSCALE_CUBIC


def _draw_photo(b, rng):
    """f7's nine entries with one seed per ENTRY (``sample_program`` draws one per slot)"""
    return draw_photo(b, rng, (b, 9))


def sample_geo_program(batch: int, preset: str, rng: np.random.Generator, h: int, w: int, interp: str = "linear") -> GeoProgram:
    """Draw the GEOMETRIC entries of one batch of a preset for ``h x w`` images, as one program (the photometric entries
    of the recipe are skipped: ``sample_heavy_plan`` interleaves both).

    ``"heavy_device"`` (``data_generator_mscmrseg.py:23-82``), 7 slots: Fliplr p = 0.5, Flipud p = 0.2, ``sometimes``
    CropAndPad (percent -0.05..0.1 per side independently, a border mode of the five, cval 0..255), ``sometimes`` Affine
    (scale 0.8-1.2 per axis, translate +/-0.2, rotate +/-45, shear +/-16 degrees, order {0, 1}, cval 0..255, a border mode of the
    five) and, out of the ``SomeOf((0, 5))`` block of twelve built entries, ``sometimes`` ElasticTransformation (alpha
    0.5-3.5, sigma 0.25), PiecewiseAffine (G = 4, jitter N(0, scale size), scale 0.01-0.05) and PerspectiveTransform (jitter
    N(0, scale), scale 0.01-0.1, clipped to 0.45), in one random order per batch.  ``"mscmrseg_aug2_device"``
    (``:89-130``), 1 slot: ``sometimes`` CropAndPad.  On ``"heavy_refpad_device"`` the six entries without CropAndPad (which is
    a ``CropPadProgram`` there, f14); ``"mscmrseg_aug2_refpad_device"`` holds no geometric entry (0 slots).  imgaug's own
    parameter stream is not reproduced (parity unpinned).  ``interp="cubic"``: every elastic slot has order 3, and one
    ``rng.random(batch)`` is consumed after every other draw (unused here: the three samplers consume alike)."""
    cubic = _check_interp(interp)
    entries, on = _select(batch, _check_preset(preset), rng)
    d = _draw_geo(batch, rng, h, w)
    if cubic:
        rng.random(batch)
    geo = [k for k, e in enumerate(entries) if e[0] == "g"]
    prog = GeoProgram.identity(batch, len(geo))
    for i in range(batch):
        s = 0
        for k in geo:
            if on[i, k]:
                _encode_geo(prog, i, s, entries[k][1], d, h, w, elastic_order=3 if cubic else 1)
                s += 1
    return prog


def sample_style_program(batch: int, preset: str, rng: np.random.Generator, h: int, w: int, interp: str = "linear") -> StyleProgram:
    """Draw the three STYLE entries of one batch of a preset (``"heavy_full_device"`` or ``"mscmrseg_aug2_full_device"``) for
    ``h x w`` images as one program of three slots, in the batch's order (the other entries of the recipe are skipped:
    ``sample_heavy_plan`` interleaves all kinds): ``sometimes(0.5)`` Superpixels (p_replace U(0, 1), n_segments 20..200 ->
    ``superpixel_grid``, 5 updates, compactness 10), SimplexNoiseAlpha (alpha U(0.5, 1), OneOf EdgeDetect | DirectedEdgeDetect
    with direction U(0, 1); 1..3 grids of 2..16 cells per side, nearest | bilinear, min | mean | max, sigmoid with a threshold
    from N(0, 5)) and AddToHueAndSaturation (v integer in -20..20: ds = v, dh = floor(v 180 / 255 + 0.5)), each only for the
    samples whose ``SomeOf((0, 5))`` drew it.  The ``_connected_`` presets draw what their ``_refpad_`` twins draw and give every
    Superpixels slot ``min_size = superpixel_min_size(gy, gx, h, w)``; the ``_scaled_`` presets draw the same again and give
    every Superpixels slot ``max_size = 128``, with the grid and ``min_size`` of ``superpixel_working_size(h, w, 128)``.
    ``interp="cubic"``: one more ``rng.random(batch)`` after
    every other draw; the SimplexNoiseAlpha slot of sample ``i`` upscales cubically where it is below ``NOISE_CUBIC_P``."""
    cubic = _check_interp(interp)
    spec = _check_preset(preset)
    entries, on = _select(batch, spec, rng)
    d = St.draw_style(batch, rng)
    cubic_draw = rng.random(batch) if cubic else None
    sty = [k for k, e in enumerate(entries) if e[0] == "s"]
    if not sty:
        raise ValueError("preset %r holds no stylize entry (have: %s, %s)" % (preset, HEAVY_FULL_PRESET, AUG2_FULL_PRESET))
    prog = StyleProgram.identity(batch, len(sty))
    for i in range(batch):
        s = 0
        for k in sty:
            if on[i, k]:
                St.encode_style(prog, i, s, entries[k][1], d, h, w, connected=bool(spec.get("connected")),
                                            scaled=bool(spec.get("scaled")))
                s += 1
    if cubic:
        _cubic_upscale(prog, cubic_draw)
    return prog


@dataclass
class HeavyPlan:
    """The ordered stages of one batch: ``PhotoProgram``, ``GeoProgram``, (f9) ``StyleProgram`` and (f14) ``CropPadProgram``
    stages, no two neighbours of one kind; every stage covers the whole batch (a sample without an active entry in a stage
    holds NOPs there)."""
    batch: int
    stages: List[Union[PhotoProgram, GeoProgram, StyleProgram, CropPadProgram]] = field(default_factory=list)

    def is_identity(self) -> bool:
        return all(st.is_identity() for st in self.stages)


def sample_heavy_plan(batch: int, preset: str, rng: np.random.Generator, h: int, w: int, interp: str = "linear") -> HeavyPlan:
    """Draw the whole recipe of one batch: photometric and geometric entries interleaved by ``random_order=True`` (one outer
    and one inner order per batch).  Consecutive photometric entries form one ``PhotoProgram``, consecutive geometric entries
    one ``GeoProgram``; a stage has as many slots as its busiest sample uses, a stage nobody uses is dropped.

    ``"heavy_device"``: ``augmentation`` minus Superpixels, SimplexNoiseAlpha and AddToHueAndSaturation -- the outer order is
    over {Fliplr, Flipud, CropAndPad, Affine, SomeOf block}; ``SomeOf`` draws 0..5 of the twelve built entries (f7's nine and
    the three warps, each warp behind ``sometimes(0.5)``).  ``"mscmrseg_aug2_device"``: ``augmentation2`` minus the same
    three -- ``sometimes(CropAndPad)`` and f7's nine-entry block, in random order.

    ``"heavy_full_device"`` and ``"mscmrseg_aug2_full_device"`` (f9): the same two recipes with all fifteen / twelve ``SomeOf``
    entries -- ``sometimes`` Superpixels, SimplexNoiseAlpha and AddToHueAndSaturation (``utils/stylize.py``) sit in the block
    at the reference's list positions, and consecutive stylize entries form one ``StyleProgram``.

    ``"heavy_refpad_device"`` and ``"mscmrseg_aug2_refpad_device"`` (f14): the two full recipes with CropAndPad as a
    ``CropPadProgram`` stage of its own (``utils/croppad.py``), its mode uniform over the ten of ``numpy.pad``.  Everything the
    ``_full_`` twin draws is drawn in the same order, then one ``rng.integers(0, 10, batch)`` for the mode; the sides and cval
    are ``_draw_geo``'s ``crop`` / ``crop_cval`` (its ``crop_mode`` draw is consumed and unused).

    ``"heavy_connected_device"`` and ``"mscmrseg_aug2_connected_device"`` (f9b): the ``_refpad_`` presets, draw for draw, with
    ``min_size = superpixel_min_size(gy, gx, h, w)`` in ``iarg[5]`` of every Superpixels slot (connected segments,
    ``csrc/spx_connect.hip``); every other array of the plan equals the ``_refpad_`` plan of the same generator state.

    ``"heavy_scaled_device"`` and ``"mscmrseg_aug2_scaled_device"`` (f9c): the ``_connected_`` presets, draw for draw, with
    ``max_size = stylize.SUPERPIXELS_MAX_SIZE`` (128, imgaug's default) in ``iarg[6]`` of every Superpixels slot
    (``csrc/spx_scale.hip``); ``iarg[0:2]`` (the grid) and ``iarg[5]`` (``min_size``) of those slots are computed for
    ``superpixel_working_size(h, w, 128)``, every other array of the plan equals the ``_connected_`` plan of the same
    generator state.

    ``interp="cubic"`` (f8b, any preset): every elastic slot has order 3 and, after every other draw of the call, one
    ``rng.random(batch)`` decides per sample whether its SimplexNoiseAlpha slot upscales cubically (below ``NOISE_CUBIC_P``);
    every other array of the plan equals the ``"linear"`` plan of the same generator state."""
    cubic = _check_interp(interp)
    spec = _check_preset(preset)
    entries, on = _select(batch, spec, rng)
    dg, dp = _draw_geo(batch, rng, h, w), _draw_photo(batch, rng)
    ds = St.draw_style(batch, rng) if any(e[0] == "s" for e in entries) else None
    pad_mode = rng.integers(0, 10, batch) if any(e[0] == "c" for e in entries) else None
    cubic_draw = rng.random(batch) if cubic else None
    used = [k for k in range(len(entries)) if on[:, k].any()]      # (an entry nobody drew does not split a stage)
    entries, on = [entries[k] for k in used], on[:, used]
    plan = HeavyPlan(batch)
    k = 0
    while k < len(entries):
        kind = entries[k][0]
        e = k
        while e < len(entries) and entries[e][0] == kind:
            e += 1
        used = int(on[:, k:e].sum(1).max()) if batch else 0
        if used:
            prog = CropPadProgram.identity(batch) if kind == "c" else _STAGE_TYPES[kind].identity(batch, used)
            for i in range(batch):
                s = 0
                for q in range(k, e):
                    if on[i, q]:
                        entry = entries[q][1]
                        if kind == "p":
                            encode_photo(prog, i, s, entry, dp, dp["seed"][i, entry])
                        elif kind == "s":
                            St.encode_style(prog, i, s, entry, ds, h, w, connected=bool(spec.get("connected")),
                                            scaled=bool(spec.get("scaled")))
                        elif kind == "c":
                            t, r, bt, l = dg["crop"][i]
                            prog.set_crop_and_pad(i, crop_pad_pixels(t, h), crop_pad_pixels(r, w), crop_pad_pixels(bt, h),
                                                  crop_pad_pixels(l, w), int(pad_mode[i]), int(dg["crop_cval"][i]))
                        else:
                            _encode_geo(prog, i, s, entry, dg, h, w, elastic_order=3 if cubic else 1)
                        s += 1
            if cubic and kind == "s":
                _cubic_upscale(prog, cubic_draw)
            plan.stages.append(prog)
        k = e
    return plan


def heavy_aug(images: torch.Tensor, masks: Optional[torch.Tensor], plan: Optional[HeavyPlan] = None):
    """Run a plan: uint8 ``[B,H,W,C]`` images and integer masks (or ``None``) on the device -> ``(images, masks)``.  ``plan``
    is required: draw it with ``sample_heavy_plan(B, "heavy_device", rng, H, W)``."""
    if plan is None:
        raise TypeError("heavy_aug: plan is required (sample_heavy_plan(batch, preset, rng, h, w)); there is no silent identity")
    if images.dtype != torch.uint8 or images.dim() != 4:
        raise TypeError("heavy_aug: uint8 [B,H,W,C] images")
    if plan.batch != images.shape[0]:
        raise ValueError("HeavyPlan for %d samples, batch of %d" % (plan.batch, images.shape[0]))
    for stage in plan.stages:
        if not isinstance(stage, tuple(_STAGE_TYPES.values())):
            raise TypeError("heavy_aug: a stage is a PhotoProgram, a GeoProgram, a StyleProgram or a CropPadProgram, got %s"
                            % type(stage).__name__)
        images, masks = stage.apply(images, masks)
    return images, masks
