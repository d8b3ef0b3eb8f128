"""bench.py's command line without a GPU: the --dump-outputs writer on host tensors (file names, dtype, size bound,
seeded sample) and the argument checks."""
import os
import subprocess
import sys
import types

import numpy as np
import torch

import bench as B

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _trainer(sizes):
    """the attributes dump_outputs reads: one flat parameter buffer per optimiser (values = their own indices)"""
    opt = lambda n: None if n is None else types.SimpleNamespace(p=torch.arange(n, dtype=torch.float32))
    return types.SimpleNamespace(opt_gen=opt(sizes[0]), opt_d1=opt(sizes[1]), opt_d2=opt(sizes[2]), opt_d4=opt(sizes[3]))


def test_dump_outputs_files_dtype_bound_and_seeded_sample(tmp_path):
    big = B.DUMP_MAX_ELEMS + 12345
    tr = _trainer([big, 1000, None, B.DUMP_MAX_ELEMS])
    out = {"loss_bce": torch.tensor(0.5), "adv2": torch.tensor([1.25])}
    B.dump_outputs(str(tmp_path / "a"), tr, out)
    names = sorted(p.name for p in (tmp_path / "a").iterdir())
    assert names == ["params_dis1.npy", "params_dis4.npy", "params_gen.npy", "step_adv2.npy", "step_loss_bce.npy"]
    arrs = {n: np.load(tmp_path / "a" / n) for n in names}
    assert all(a.dtype == np.float32 for a in arrs.values())
    assert sum((tmp_path / "a" / n).stat().st_size for n in names) <= 64 << 20
    assert arrs["step_loss_bce.npy"].tolist() == [0.5] and arrs["step_adv2.npy"].tolist() == [1.25]
    assert np.array_equal(arrs["params_dis1.npy"], np.arange(1000, dtype=np.float32))        # small buffers: whole
    assert np.array_equal(arrs["params_dis4.npy"], np.arange(B.DUMP_MAX_ELEMS, dtype=np.float32))
    g = arrs["params_gen.npy"]             # a sample: DUMP_MAX_ELEMS distinct indices, sorted
    assert g.size == B.DUMP_MAX_ELEMS and np.all(np.diff(g) > 0) and g[-1] < big
    B.dump_outputs(str(tmp_path / "b"), tr, out)                     # the same indices in every run
    assert np.array_equal(np.load(tmp_path / "b" / "params_gen.npy"), g)


def test_bench_refuses_zero_steps_and_lists_its_options():
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--steps", "0", "--dry-run"],
                       capture_output=True, text=True, timeout=120)
    assert r.returncode == 2 and "--steps" in r.stderr and '"metric"' not in r.stdout
    h = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--help"], capture_output=True, text=True, timeout=120)
    assert h.returncode == 0 and "--full" in h.stdout and "--dump-outputs" in h.stdout
