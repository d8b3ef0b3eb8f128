"""bench.py on the GPU: a plain run prints the contract fields and nothing that --full adds, --steps sets the number of
timed steps, and --dump-outputs writes the same outputs in two runs with the same arguments."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FULL_ONLY = ("host_issue_ms_per_step", "launches_per_step", "comm_exposed_ms", "clock_ghz_under_load", "img_s_per_ghz",
             "roofline", "cpu_baseline")


def _run(out_dir):
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "3", "--warmup", "1",
                        "--settle", "1", "--dump-outputs", out_dir], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    return json.loads(r.stdout.strip().splitlines()[-1])


@pytest.mark.gpu
def test_plain_bench_line_and_dumped_outputs(dev, tmp_path):
    a, b = str(tmp_path / "a"), str(tmp_path / "b")
    res = _run(a)
    assert res["steps"] == 3 and res["warmup"] == 1 and res["unit"] == "img/s" and res["higher_is_better"] is True
    assert res["value"] > 0 and res["ms_per_step"] > 0 and isinstance(res["metric"], str) and isinstance(res["dtype"], str)
    assert abs(res["value"] - res["config"]["global_batch"] * 1000.0 / res["ms_per_step"]) <= 0.01 * res["value"]
    assert not [k for k in FULL_ONLY if k in res], res.keys()
    names = sorted(os.listdir(a))
    assert {"step_loss_bce.npy", "step_loss_jac.npy", "params_gen.npy", "params_dis1.npy", "params_dis2.npy",
            "params_dis4.npy"} <= set(names), names
    assert sum(os.path.getsize(os.path.join(a, n)) for n in names) <= 64 << 20
    first = {n: np.load(os.path.join(a, n)) for n in names}
    assert all(v.dtype in (np.float32, np.float64) and v.size and np.all(np.isfinite(v)) for v in first.values())
    _run(b)
    assert sorted(os.listdir(b)) == names
    for n in names:
        np.testing.assert_allclose(np.load(os.path.join(b, n)), first[n], rtol=1e-5, atol=1e-7, err_msg=n)
