"""Evaluation metrics on the HIP kernels (surface_metrics, largest_components and the medpy / reference names built on
them) against tests/golden/eval_metrics.npz (scipy restatement, scripts/make_eval_golden.py) and, for label maps made
on the device, the numpy brute-force restatement of the same definitions."""
import importlib.util
import os
import types

import numpy as np
import pytest
import torch

from conftest import GOLD, ROOT

# the numpy-only half of the restatement (blobs, brute force), loaded by path: scripts/ stays off sys.path
_spec = importlib.util.spec_from_file_location("make_eval_golden", os.path.join(ROOT, "scripts", "make_eval_golden.py"))
G = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(G)

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def gold():
    return np.load(os.path.join(GOLD, "eval_metrics.npz"))


def _surface_cases(g):
    i = 0
    while "s%d_name" % i in g.files:
        p = "s%d_" % i
        if p + "regen" in g.files:
            pred, gt = G.big_volume()
        else:
            pred, gt = g[p + "pred"], g[p + "gt"]
        sp = g[p + "spacing"]
        yield str(g[p + "name"]), pred, gt, [int(c) for c in g[p + "classes"]], (tuple(sp) if sp.size else None), \
            int(g[p + "conn"]), g[p + "out"]
        i += 1


def _check_rows(got, exp, name, exact_hd):
    assert np.array_equal(got[:, [0, 4, 5, 6, 7]], exp[:, [0, 4, 5, 6, 7]]), (name, got, exp)     # dice and counts: exact
    empty = exp[:, 7] != 0
    assert np.isnan(got[empty, 1:4]).all(), name
    if exact_hd:
        assert np.array_equal(got[~empty, 1], exp[~empty, 1]), (name, got[:, 1], exp[:, 1])
    else:
        assert np.allclose(got[~empty, 1], exp[~empty, 1], rtol=1e-12, atol=0), (name, got[:, 1], exp[:, 1])
    assert np.allclose(got[~empty, 2:4], exp[~empty, 2:4], rtol=1e-12, atol=0), (name, got[:, 2:4], exp[:, 2:4])


def test_surface_metrics_against_the_fixture(dev, gold):
    from pointcloududa_amd import kernels as K
    n = 0
    for name, pred, gt, cls, sp, conn, exp in _surface_cases(gold):
        tp, tg = torch.from_numpy(np.ascontiguousarray(pred)).to(dev), torch.from_numpy(np.ascontiguousarray(gt)).to(dev)
        out = K.surface_metrics(tp, tg, cls, sp, conn)
        assert out.dtype == torch.float64 and out.is_cuda and out.shape == (len(cls), 8)
        got = out.cpu().numpy()
        _check_rows(got, exp, name, exact_hd=sp is None)
        again = K.surface_metrics(tp, tg, cls, sp, conn).cpu().numpy()
        assert np.array_equal(got.view(np.int64), again.view(np.int64)), name          # the same bits, run to run
        if pred.max() < 256 and pred.min() >= 0:                                           # uint8 labels: same results
            got8 = K.surface_metrics(tp.to(torch.uint8), tg.to(torch.uint8), cls, sp, conn).cpu().numpy()
            assert np.array_equal(got.view(np.int64), got8.view(np.int64)), name
        n += 1
    assert n >= 19


def test_medpy_wrappers(dev, gold):
    from pointcloududa_amd.utils import metric as M
    for name, pred, gt, cls, sp, conn, exp in _surface_cases(gold):
        if pred.size > 200000:
            continue
        c, row = cls[0], exp[0]
        a, b = (pred == c), (gt == c)
        ta = torch.from_numpy(a.astype(np.uint8)).to(dev)
        assert M.dc(a, b) == row[0] and M.dc(ta, b) == row[0]
        if row[7]:
            msg = G_MSG[int(row[7]) & 1 == 0]
            with pytest.raises(RuntimeError, match=msg):
                M.hd(a, b, sp, conn)
            with pytest.raises(RuntimeError, match=msg):
                M.asd(ta, b, sp, conn)
            continue
        h = M.hd(a, b, sp, conn)
        assert isinstance(h, float) and (h == row[1] if sp is None else abs(h - row[1]) <= 1e-12 * row[1]), name
        assert abs(M.asd(a, b, sp, conn) - row[2]) <= 1e-12 * row[2], name
        assert abs(M.asd(b, ta, sp, conn) - row[3]) <= 1e-12 * row[3], name


G_MSG = {False: "first supplied array", True: "second supplied array"}


def test_largest_components_against_the_fixture(dev, gold):
    from pointcloududa_amd import kernels as K
    from pointcloududa_amd.utils.utils import keep_largest_connected_components
    i = 0
    while "c%d_name" % i in gold.files:
        m, exp = gold["c%d_mask" % i], gold["c%d_out" % i]
        got = K.largest_components(torch.from_numpy(m).to(dev))
        assert got.dtype == torch.uint8 and np.array_equal(got.cpu().numpy(), exp), str(gold["c%d_name" % i])
        got_np = keep_largest_connected_components(m.astype(np.int64))
        assert isinstance(got_np, np.ndarray) and np.array_equal(got_np, exp)
        i += 1
    assert i >= 5
    with pytest.raises(ValueError, match="uint8"):
        bad = np.zeros((2, 300, 4), np.int32); bad[0, 0, 0] = 260
        keep_largest_connected_components(bad)
    with pytest.raises(ValueError, match="uint8"):
        keep_largest_connected_components(torch.from_numpy(bad).to(dev))
    big = np.zeros((2, 300, 4), np.int32); big[0, 0, :2] = 300 + 5                      # above shape[1]: ignored, as the reference
    assert not keep_largest_connected_components(big).any()


def test_compute_metrics_on_files(dev, gold, capsys):
    from pointcloududa_amd import evaluate_mmwhs as EW
    from pointcloududa_amd import evaluate_mscmrseg as EM
    i = 0
    while "f%d_variant" % i in gold.files:
        p = "f%d_" % i
        mod = EM if str(gold[p + "variant"]) == "mscmrseg" else EW
        ifhd, ifasd = (bool(v) for v in gold[p + "flags"])
        res = mod.compute_metrics_on_files(gold[p + "gt"], gold[p + "pred"], ifhd=ifhd, ifasd=ifasd)
        exp = gold[p + "res"]
        assert len(res) == len(exp)
        for r, e in zip(res, exp):
            assert r == e or abs(r - e) <= 1e-12 * abs(e), (i, res, exp)
        assert capsys.readouterr().out.count(" , ") == len(exp) - 1
        i += 1
    assert i >= 6


def test_evaluate_and_metrics2_raise_like_medpy(dev, gold):
    from pointcloududa_amd.utils import metric as M
    gt = G.blobs((6, 32, 32), 71, [1, 2, 3, 4]).astype(np.uint8)
    pred = G.blobs((6, 32, 32), 71, [1, 2, 3, 4], shift=2).astype(np.uint8)
    r = M.metrics2(gt, pred, apply_hd=True, apply_asd=True)
    exp = G.surface_brute(gt, pred, [1, 2, 3, 4])
    for k, name in enumerate(["myo", "la", "lv", "aa"]):
        assert r[name][0] == exp[k, 0] and r[name][1] == exp[k, 1] and abs(r[name][2] - exp[k, 2]) <= 1e-12 * exp[k, 2]
    assert M.evaluate(gt, pred)["lv"][1:] == [0, 0]
    pe = pred.copy(); pe[pe == 2] = 0
    assert M.evaluate(gt, pe)["lv"][0] == 0.0                                            # dice only: no error
    with pytest.raises(RuntimeError, match="second supplied array"):
        M.evaluate(gt, pe, apply_hd=True)
    with pytest.raises(RuntimeError, match="first supplied array"):
        M.metrics2(pe, gt, apply_asd=True)


def _stub_model(dev, n_class):
    """a 'segmenter' whose logits put every pixel in the class of its intensity band: all classes present"""
    class Stub(torch.nn.Module):
        def __init__(self):
            super().__init__()
            self.w = torch.nn.Parameter(torch.ones(1))

        def forward(self, x):
            centres = torch.linspace(0, 1, n_class, device=x.device).view(1, -1, 1, 1)
            return (-(x[:, :1] - centres) ** 2 * self.w).contiguous(), None, None
    return Stub().to(dev)


def _batches(n_class, seed, nb=3, b=3, hw=48):
    rng = np.random.default_rng(seed)
    out = []
    for i in range(nb):
        x = np.stack([G.blobs((hw, hw), seed + 7 * i + j, [1, 2, 3, 4, 5][:n_class - 1], n=10) for j in range(b)])
        x = (x / (n_class - 1) + rng.normal(0, 0.08, x.shape)).astype(np.float32)[:, None]
        lab = np.stack([G.blobs((hw, hw), seed + 7 * i + j, [1, 2, 3, 4, 5][:n_class - 1], n=10, shift=2) for j in range(b)])
        y = np.moveaxis(np.eye(n_class, dtype=np.uint8)[lab], -1, 1).copy()
        out.append((x, y, np.zeros((b, 300, 3), np.float32)))
    return out


@pytest.mark.parametrize("variant", ["mscmrseg", "mmwhs"])
def test_valid_model_with_one_dataset_hd(dev, variant):
    import pointcloududa_amd.train_mmwhs as TW
    import pointcloududa_amd.train_mscmrseg as TM
    from pointcloududa_amd.utils import metric as M
    n_class = 4 if variant == "mscmrseg" else 5
    model = _stub_model(dev, n_class)
    batches = _batches(n_class, 80 if variant == "mscmrseg" else 90)
    T = TM if variant == "mscmrseg" else TW
    args = types.SimpleNamespace(d1=False, d2=True, d4=False, d4aux=False, softmax=True)
    res = T.valid_model_with_one_dataset(model, iter(batches), hd=True, args=args)
    plain = T.valid_model_with_one_dataset(model, iter(batches), hd=False, args=args)
    assert set(res) == set(plain) | {"hd"} and all(res[k] == plain[k] for k in plain)
    cls = [1, 2, 3] if variant == "mscmrseg" else [1, 2, 3, 4]
    order = [1, 0, 2] if variant == "mscmrseg" else [2, 0, 1, 3]
    hd_list = []
    for x, y, _ in batches:
        with torch.no_grad():
            pred = M.argmax_labels(model(torch.from_numpy(x).to(dev))[0]).cpu().numpy()
        rows = G.surface_brute(np.argmax(y, axis=1), pred, cls)                   # the batch as one [B,H,W] volume
        assert not rows[:, 7].any()
        hd_list.append(sum(rows[k, 1] for k in order) / float(len(cls)))
    assert res["hd"] == np.mean(np.array(hd_list))
    # a class missing from one batch's prediction: medpy's error, raised at the data set's synchronisation
    bad = [list(bt) for bt in batches]
    bad[1][0] = np.full_like(bad[1][0], 0.0)
    with pytest.raises(RuntimeError, match="second supplied array"):
        T.valid_model_with_one_dataset(model, iter([tuple(bt) for bt in bad]), hd=True, args=args)


def test_valid_model_hd_with_the_segmenter(dev):
    """the real network: hd (or medpy's error) as the brute-force restatement gives it on the same label maps"""
    from oracle import nets as ON
    from oracle.synth import synth_batch
    import pointcloududa_amd.train_mscmrseg as TM
    from pointcloududa_amd.networks import Segmentation_model_Point
    from pointcloududa_amd.utils import metric as M
    kw = dict(filters=4, in_channels=1, n_class=4, pointnet=True, fc_inch=9)
    m = Segmentation_model_Point(**kw)
    m.load_state_dict({k: v.clone() for k, v in ON.make_params(ON.seg_param_shapes(ON.SegCfg(**kw)), 2700).items()})
    m = m.to(dev)
    batches = [synth_batch(2, 1, 4, 128, seed=2710 + i)[:3] for i in range(2)]
    args = types.SimpleNamespace(d1=False, d2=True, d4=True, dr=0.01, wp=1.0)
    err, hd_list = None, []
    m.eval()
    for x, y, _ in batches:
        with torch.no_grad():
            pred = M.argmax_labels(m(torch.from_numpy(x).to(dev))[0]).cpu().numpy()
        rows = G.surface_brute(np.argmax(y, axis=1), pred, [1, 2, 3])
        for r in rows:
            if r[7] and err is None:
                err = G_MSG[int(r[7]) & 1 == 0]
        hd_list.append((rows[1, 1] + rows[0, 1] + rows[2, 1]) / 3.0)
    if err is not None:
        with pytest.raises(RuntimeError, match=err):
            TM.valid_model_with_one_dataset(m, iter(batches), hd=True, args=args)
    else:
        assert TM.valid_model_with_one_dataset(m, iter(batches), hd=True, args=args)["hd"] == np.mean(np.array(hd_list))


@pytest.mark.parametrize("variant", ["mmwhs", "mscmrseg"])
def test_evaluate_volume_matches_the_host_path(dev, variant):
    from pointcloududa_amd import validate as V
    from pointcloududa_amd.utils import metric as M
    n_class = 5 if variant == "mmwhs" else 4
    model = _stub_model(dev, n_class)
    x = np.concatenate([b[0] for b in _batches(n_class, 100, nb=2, b=5, hw=40)])             # a 10-slice volume
    gt = np.concatenate([np.argmax(b[1], axis=1) for b in _batches(n_class, 100, nb=2, b=5, hw=40)])
    with torch.no_grad():
        pred = M.argmax_labels(model(torch.from_numpy(x).to(dev))[0]).cpu().numpy()
    pred = G.largest_components_brute(pred)
    if variant == "mscmrseg":
        lut = np.array([0, 200, 500, 600]); pred, gt = lut[pred], lut[gt]
        cls = [500, 600, 200]
    else:
        cls = [1, 2, 3, 4]
    rows = G.surface_brute(gt, pred, cls)
    exp = (G.mscmrseg_list if variant == "mscmrseg" else G.mmwhs_list)(rows, True, True)
    got = V.evaluate_volume(model, x, gt, bs=4, klc=True, ifhd=True, ifasd=True, variant=variant)
    assert len(got) == len(exp)
    for r, e in zip(got, exp):
        assert r == e or abs(r - e) <= 1e-12 * abs(e), (got, exp)
