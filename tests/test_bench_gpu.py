"""bench.py on the device: a plain run prints the headline line only (no roofline, no baselines: those are `--full`) and
`--dump-outputs` writes what the last timed step computed -- the solution, dL/dy0 and the six parameter gradients at the
shapes the step returns them -- as float32, within 64 MB."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import ROOT

pytestmark = pytest.mark.gpu


def test_plain_run_prints_the_headline_and_dumps_the_last_step(tmp_path):
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "LOCAL_RANK", "WORLD_SIZE", "MASTER_ADDR", "MASTER_PORT")}
    out = tmp_path / "outputs"
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "3", "--warmup", "1",
                        "--prewarm-seconds", "0.05", "--dump-outputs", str(out)],
                       env=env, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=300, cwd=ROOT)
    assert r.returncode == 0, r.stderr.decode()[-3000:]
    lines = [ln for ln in r.stdout.decode().splitlines() if ln.strip()]
    assert len(lines) == 1, lines
    d = json.loads(lines[0])
    assert d["steps"] == 3 and d["warmup"] == 1 and d["n_gpus"] == 1
    assert d["metric"] == "ODE-RHS evals/sec (genes x trajectories)" and d["unit"] == "gene*trajectory RHS evals/s"
    assert d["higher_is_better"] is True and d["dtype"] == "f32" and d["value"] > 0 and d["ms_per_step"] > 0
    assert "roofline" not in d and "cpu_baseline" not in d and "training_step_ms" not in d
    N, H, B = d["config"]["genes"], d["config"]["hidden"], d["config"]["trajectories_per_gpu"]
    T = len(d["config"]["time_points"])
    want = {"solution": (T, B, 1, N), "grad_y0": (B, 1, N),
            "grad_net_prods_linear_out_weight": (H, N), "grad_net_prods_linear_out_bias": (H,),
            "grad_net_sums_linear_out_weight": (H, N), "grad_net_sums_linear_out_bias": (H,),
            "grad_net_alpha_combine_linear_out_weight": (N, 2 * H), "grad_gene_multipliers": (1, N)}
    assert sorted(f[:-4] for f in os.listdir(out) if f.endswith(".npy")) == sorted(want)
    assert sum(os.path.getsize(str(out / f)) for f in os.listdir(out)) <= 64 * 10 ** 6
    for name, shape in want.items():
        a = np.load(str(out / (name + ".npy")))
        assert a.dtype == np.float32 and a.shape == shape and np.isfinite(a).all(), (name, a.dtype, a.shape)
        assert np.abs(a).max() > 0, name
