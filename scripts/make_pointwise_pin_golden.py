"""Pins every output bit of the BatchNorm / LeakyReLU / pooling / point-max family (csrc/pointwise.hip,
csrc/pointnet_small.hip) in tests/golden/pointwise_pin.json; tests/test_pointwise_pin_gpu.py compares a build to it.

Run it on the build whose behaviour is to be kept (the PARENT of a refactor), never on the commit under test:

    python scripts/make_pointwise_pin_golden.py [--out tests/golden/pointwise_pin.json]        # needs the MI355X

It calls only the public functions of pointcloududa_amd.kernels, so the same file runs on either side of a refactor.  One
record per case (scripts/pin_common.py): the ``launch_count()`` delta of every call, the sha256 of the raw bytes of every
output tensor (statistics, running buffers, activations, gradients, partials) and of the inputs, folded per case into one
digest of the outputs and one of the inputs (``fold``; ``record(dev, folded=False)`` names the tensor that moved).

Inputs: ``np.random.default_rng`` with a seed derived from the case key, normal(0, 1) values, nothing moved away from the
ReLU / LeakyReLU gates.  The shapes are the smallest at which each branch of the kernels and their dispatch is taken: one
element, one tile of 2048 exactly, one element and one vector past it, several tiles and samples, planes that fail the
float4 test (33 x 33, hw = 5), more tiles than the finalize kernels' unrolled loop takes in one trip (3900)."""
from __future__ import annotations

import hashlib
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from pin_common import ROOT, K, _counted, _seed, _sha, recorder_main, unique_cases  # noqa: E402

OUT = os.path.join(ROOT, "tests", "golden", "pointwise_pin.json")

PLANE_SHAPES = ((1, 1, 1), (2, 1, 1), (1, 3, 2048), (1, 3, 2049), (1, 3, 2052), (2, 3, 4100), (3, 5, 33, 33), (1800, 2, 5),
                (3900, 1, 4))
# dense; channels 1 .. 1 + c of a tensor two channels wider; a dense tensor whose base is 4 bytes past a 16-byte boundary
LAYOUTS = ("dense", "slice", "off4")
RED_SHAPES = ((2, 3, 8, 10), (1, 2, 46, 46))
POOLED_SHAPES = ((1, 1, 2, 2), (2, 3, 6, 4), (2, 3, 6, 6), (1, 2, 64, 64))
LRELU_CASES = (("vec", (2, 3, 8, 8), "dense"), ("flat", (4, 3, 5, 7), "dense"), ("scalar", (1, 3, 5, 7), "dense"),
               ("slice", (2, 3, 8, 8), "slice"))
BN1D_B = (1, 2, 17, 256, 257, 1024, 1025)      # 1025: past the one-launch kernels, the general path
BN1D_C = (1, 16, 17)
MAXPTS_SHAPES = ((2, 3, 1), (2, 17, 7), (3, 5, 2048), (2, 3, 2052))      # 2052: past one tile, the dense fallback
CSUM_SHAPES = ((1, 3, 2047), (1, 3, 2048), (2, 3, 2049))


class _Draw:
    """tensors of one case: drawn on the host from the case's seed, hashed, placed on the device in a layout"""

    def __init__(self, dev, *key):
        self.dev, self.rng, self.ins = dev, np.random.default_rng(_seed(*key)), {}

    def host(self, name, shape, dtype=np.float32):
        t = torch.from_numpy(self.rng.normal(0, 1.0, shape).astype(dtype))
        self.ins[name] = _sha(t)
        return t

    def __call__(self, name, shape, layout="dense"):
        t = self.host(name, shape)
        if layout == "dense":
            return t.to(self.dev)
        if layout == "slice":
            wide = torch.zeros((shape[0], shape[1] + 2) + tuple(shape[2:]), dtype=torch.float32, device=self.dev)
            view = wide[:, 1:1 + shape[1]]
        elif layout == "off4":
            view = torch.zeros(t.numel() + 1, dtype=torch.float32, device=self.dev)[1:].view(shape)
        elif layout == "odd":      # planes one element apart from dense: odd batch / channel strides for even planes
            hw = int(np.prod(shape[2:]))
            buf = torch.zeros((shape[0], shape[1], hw + 1), dtype=torch.float32, device=self.dev)
            view = torch.as_strided(buf, shape, (shape[1] * (hw + 1), hw + 1) + tuple(torch.empty(shape[2:]).stride()))
        elif layout == "rows":     # [B, C] rows three elements wider than C
            view = torch.zeros((shape[0], shape[1] + 3), dtype=torch.float32, device=self.dev)[:, :shape[1]]
        else:
            raise ValueError(layout)
        view.copy_(t)
        return view


def _affine(draw, c):
    """gamma, beta, running mean, running variance of a layer"""
    gamma, beta, rm = draw("gamma", (c,)), draw("beta", (c,)), draw("rm", (c,))
    return gamma, beta, rm, draw("rv", (c,)).abs() + 0.5


def _state_hashes(st, tag=""):
    return {tag + k: _sha(getattr(st, k)) for k in ("mean", "invstd", "scale", "shift")}


def _forward(launches, a, gamma, beta, rm=None, rv=None):
    """bn_stats -> bn_finalize: the BNState the backward cases start from"""
    partials, nt, count = _counted(launches, "stats", lambda: K.bn_stats(a))
    st = _counted(launches, "finalize", lambda: K.bn_finalize(partials, nt, count, gamma, beta, rm, rv))
    return partials, st


def _name(shape):
    return "x".join(str(d) for d in shape)


def _flags(**kw):
    return "".join("/" + k for k, v in kw.items() if v)


def forward_cases(dev):
    for shape in PLANE_SHAPES:
        for layout in LAYOUTS:
            key = "fwd/%s/%s" % (_name(shape), layout)
            draw, launches = _Draw(dev, key), {}
            a = draw("a", shape, layout)
            gamma, beta, rm, rv = _affine(draw, shape[1])
            partials, st = _forward(launches, a, gamma, beta)
            h = {"partials": _sha(partials), **_state_hashes(st)}
            _, st_run = _forward(launches, a, gamma, beta, rm, rv)
            h.update(_state_hashes(st_run, "run_"), rm=_sha(rm), rv=_sha(rv))
            for relu in (False, True):
                for fma in (False, True):
                    name = "apply%s" % _flags(relu=relu, fma=fma)
                    h[name] = _sha(_counted(launches, name, lambda: K.bn_apply(a, st, relu=relu, fma=fma)))
            out = draw("out", shape, layout)      # into a tensor of the input's layout
            _counted(launches, "apply_out", lambda: K.bn_apply(a, st, relu=True, out=out))
            h["apply_out"] = _sha(out)
            yield {"case": key, "launches": launches, "in": draw.ins, "hash": h}


def _backward(draw, launches, h, name, call, c, accumulate):
    """one backward call with fresh dgamma / dbeta (pre-filled: ``accumulate`` adds to them); hashes dz and both"""
    dgamma, dbeta = draw("dgamma_" + name, (c,)), draw("dbeta_" + name, (c,))
    h["dz_" + name] = _sha(_counted(launches, name, lambda: call(dgamma, dbeta, accumulate)))
    h["dgamma_" + name], h["dbeta_" + name] = _sha(dgamma), _sha(dbeta)


def backward_cases(dev):
    for shape in PLANE_SHAPES:
        for layout in LAYOUTS:
            key = "bwd/%s/%s" % (_name(shape), layout)
            draw, launches, h = _Draw(dev, key), {}, {}
            c = shape[1]
            a, dy, dy2 = draw("a", shape, layout), draw("dy", shape, layout), draw("dy2", shape, layout)
            gamma, beta, _, _ = _affine(draw, c)
            _, st = _forward(launches, a, gamma, beta)
            # the full cross on dense tensors; strided and misaligned ones change the dispatch only
            cross = [(pr, two, acc, fr) for pr in (0, 1) for two in (0, 1) for acc in (0, 1) for fr in (0, 1)]
            for pr, two, acc, fr in cross if layout == "dense" else [(0, 1, 1, 0), (1, 0, 0, 1)]:
                name = "bn%s" % _flags(post_relu=pr, dy2=two, accumulate=acc, frozen=fr)
                _backward(draw, launches, h, name, lambda dg, db, ac: K.bn_backward(
                    dy, a, st, gamma, dg, db, dy2=dy2 if two else None, post_relu=bool(pr), act_slope=0.2,
                    accumulate=ac, frozen=bool(fr)), c, bool(acc))
            _backward(draw, launches, h, "bn/nogamma", lambda dg, db, ac: K.bn_backward(dy, a, st, None, None, None), c, True)
            yield {"case": key, "launches": launches, "in": draw.ins, "hash": h}
    for shape in RED_SHAPES:      # partials from the 2x2 fold's epilogue
        key = "bwd_red/%s" % _name(shape)
        draw, launches, h = _Draw(dev, key), {}, {}
        n, c, hh, ww = shape
        a, dy = draw("a", shape), draw("dy", (n, c, 2 * hh, 2 * ww))
        gamma, beta, _, _ = _affine(draw, c)
        _, st = _forward(launches, a, gamma, beta)
        dx, red = _counted(launches, "fold", lambda: K.upsample2_bwd(dy, bnred=(a, st)))
        h["dx"] = _sha(dx)
        if red is not None:
            h["red"] = _sha(red[0])
        for acc in (0, 1):
            _backward(draw, launches, h, "bn%s" % _flags(accumulate=acc), lambda dg, db, ac: K.bn_backward(
                dx, a, st, gamma, dg, db, act_slope=0.2, accumulate=ac, red=red), c, bool(acc))
        yield {"case": key, "launches": launches, "in": draw.ins, "hash": h}


def pooled_cases(dev):
    for shape in POOLED_SHAPES:
        for glayout in ("dense", "odd"):
            key = "pooled/%s/g-%s" % (_name(shape), glayout)
            draw, launches, h = _Draw(dev, key), {}, {}
            n, c, hh, ww = shape
            half = (n, c, hh // 2, ww // 2)
            a, dy = draw("a", shape), draw("dy", shape)
            g, g2 = draw("g", half, glayout), draw("g2", half, glayout)
            gamma, beta, _, _ = _affine(draw, c)
            _, idx = _counted(launches, "maxpool", lambda: K.maxpool2_fwd(draw("pooled_from", shape)))
            h["idx"] = _sha(idx)
            _, st = _forward(launches, a, gamma, beta)
            for two in (0, 1):
                for full in (0, 1):
                    kw = dict(g2=g2 if two else None, dy=dy if full else None)
                    name = "lrelu%s" % _flags(g2=two, dy=full)
                    h[name] = _sha(_counted(launches, name, lambda: K.lrelu_bwd_pooled(g, idx, a, 0.2, **kw)))
                    for fr in (0, 1):
                        _backward(draw, launches, h, "bn%s" % _flags(g2=two, dy=full, frozen=fr),
                                  lambda dg, db, ac: K.bn_backward_pooled(g, idx, a, st, gamma, dg, db, act_slope=0.2,
                                                                          accumulate=ac, frozen=bool(fr), **kw), c, bool(full))
            yield {"case": key, "launches": launches, "in": draw.ins, "hash": h}


def lrelu_cases(dev):
    for tag, shape, layout in LRELU_CASES:
        key = "lrelu/%s/%s" % (tag, _name(shape))
        draw, launches, h = _Draw(dev, key), {}, {}
        a, dy, dy2 = draw("a", shape, layout), draw("dy", shape, layout), draw("dy2", shape, layout)
        h["one"] = _sha(_counted(launches, "one", lambda: K.lrelu_bwd(dy, a, 0.2)))
        h["two"] = _sha(_counted(launches, "two", lambda: K.lrelu_bwd(dy, a, 0.2, dy2=dy2)))
        yield {"case": key, "launches": launches, "in": draw.ins, "hash": h}


def bn1d_cases(dev):
    for b in BN1D_B:
        for c in BN1D_C:
            for layout in ("dense", "rows"):
                key = "bn1d/%dx%d/%s" % (b, c, layout)
                draw, launches, h = _Draw(dev, key), {}, {}
                a, dy = draw("a", (b, c), layout), draw("dy", (b, c), layout)
                gamma, beta, rm, rv = _affine(draw, c)
                for relu in (False, True):
                    tag = "relu_" if relu else ""
                    got = _counted(launches, tag + "fwd", lambda: K.bn1d_forward(a, gamma, beta, rm, rv, relu=relu))
                    if got is None:      # what the networks do where the one-launch kernel does not apply
                        _, st = _forward(launches, a, gamma, beta, rm, rv)
                        y = _counted(launches, tag + "apply", lambda: K.bn_apply(a, st, relu=relu))
                    else:
                        st, y = got
                    h.update(_state_hashes(st, tag), **{tag + "y": _sha(y), tag + "rm": _sha(rm), tag + "rv": _sha(rv)})
                    for acc in (0, 1):
                        _backward(draw, launches, h, "bn%s" % _flags(post_relu=relu, accumulate=acc),
                                  lambda dg, db, ac: K.bn_backward(dy, a, st, gamma, dg, db, post_relu=relu, act_slope=0.2,
                                                                   accumulate=ac), c, bool(acc))
                yield {"case": key, "launches": launches, "in": draw.ins, "hash": h}


def maxpts_cases(dev):
    for shape in MAXPTS_SHAPES:
        key = "maxpts/%s" % _name(shape)
        draw, launches, h = _Draw(dev, key), {}, {}
        b, c, l = shape
        a, g = draw("a", shape), draw("g", (b, c))
        gamma, beta, _, _ = _affine(draw, c)
        _, st = _forward(launches, a, gamma, beta)
        for pr in (0, 1):
            y = K.bn_apply(a, st, relu=bool(pr))
            y[0, 0, :] = float("nan")      # a row without a maximum: idx names no element
            _, idx = _counted(launches, "max%s" % _flags(post_relu=pr), lambda: K.max_points_fwd(y))
            h["idx%s" % _flags(post_relu=pr)] = _sha(idx)
            for fr in (0, 1):
                for acc in (0, 1):
                    _backward(draw, launches, h, "bn%s" % _flags(post_relu=pr, frozen=fr, accumulate=acc),
                              lambda dg, db, ac: K.bn_backward_maxpts(g, idx, a, st, gamma, dg, db, post_relu=bool(pr),
                                                                      act_slope=0.2, accumulate=ac, frozen=bool(fr)), c, bool(acc))
        yield {"case": key, "launches": launches, "in": draw.ins, "hash": h}


def channel_sum_cases(dev):
    for shape in CSUM_SHAPES:
        key = "channel_sum/%s" % _name(shape)
        draw, launches, h = _Draw(dev, key), {}, {}
        dz = draw("dz", shape)
        for acc in (False, True):
            db = draw("db%d" % acc, (shape[1],))
            _counted(launches, "sum%d" % acc, lambda: K.channel_sum(dz, db, accumulate=acc))
            h["db%d" % acc] = _sha(db)
        yield {"case": key, "launches": launches, "in": draw.ins, "hash": h}


def neighbour_cases(dev):
    """the kernels of the same source file that the refactor leaves alone, one case each"""
    key = "neighbours"
    draw, launches, h = _Draw(dev, key), {}, {}
    x, g = draw("x", (2, 3, 6, 8)), draw("g", (2, 3, 3, 4))
    y, idx = _counted(launches, "maxpool2_fwd", lambda: K.maxpool2_fwd(x))
    h.update(pool_y=_sha(y), pool_idx=_sha(idx))
    h["maxpool2_bwd"] = _sha(_counted(launches, "maxpool2_bwd", lambda: K.maxpool2_bwd(g, idx, 6, 8)))
    h["upsample2_bwd"] = _sha(_counted(launches, "upsample2_bwd", lambda: K.upsample2_bwd(x)))
    up = _counted(launches, "bilinear_fwd", lambda: K.bilinear_fwd(x, 11, 13))
    h["bilinear_fwd"] = _sha(up)
    h["bilinear_bwd"] = _sha(_counted(launches, "bilinear_bwd", lambda: K.bilinear_bwd(up, 6, 8)))
    h["unfold_taps"] = _sha(_counted(launches, "unfold_taps", lambda: K.unfold_taps(x, 4, 2, 1)))
    x2, x3 = draw("x2", (2, 3, 6, 8)), draw("x3", (2, 3, 6, 8))
    h["add_n"] = _sha(_counted(launches, "add_n", lambda: K.add_n([x, x2, x3])))
    h["mul"] = _sha(_counted(launches, "mul", lambda: K.mul(x, x2)))
    yield {"case": key, "launches": launches, "in": draw.ins, "hash": h}


def fold(hashes):
    """{name: sha256} -> one entry: the sha256 over the sorted (name, sha256) pairs, keyed by how many there are.  A case has
    up to 60 tensors; the fixture keeps one digest of its inputs and one of its outputs, which differ as soon as one does."""
    text = json.dumps(sorted(hashes.items()), separators=(",", ":"))
    return {"sha256_of_%d" % len(hashes): hashlib.sha256(text.encode()).hexdigest()}


def record(dev, folded=True):
    """the records of every case, in a fixed order, of the library pointcloududa_amd._lib loads; ``folded=False`` keeps the
    hash of every tensor by name (to find WHICH output of a case moved)"""
    out = []
    for cases in (forward_cases, backward_cases, pooled_cases, lrelu_cases, bn1d_cases, maxpts_cases, channel_sum_cases,
                  neighbour_cases):
        out += list(cases(dev))
    torch.cuda.synchronize(dev)
    if folded:
        out = [dict(r, **{"in": fold(r["in"]), "hash": fold(r["hash"])}) for r in out]
    return unique_cases(out)


def main(argv):
    recorder_main("make_pointwise_pin_golden", argv, OUT,
                  "output hashes and launch counts of the BatchNorm / LeakyReLU / pooling family on the parent of the "
                  "one-gradient-source refactor (scripts/make_pointwise_pin_golden.py)", record)


if __name__ == "__main__":
    main(sys.argv[1:])
