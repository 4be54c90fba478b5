"""bench.py's multi-rank plumbing without a GPU: `--gpus 2` with no launcher in the environment must start two ranks
itself and rank 0 must print ONE JSON line saying n_gpus = 2 (the flag used to be parsed and ignored).
The gloo backend swaps the engine for a CPU stub -- the line says so and carries no value.  Also the parts of
`--dump-outputs` that need no GPU: seeded inputs and the writer of the arrays."""
import json
import os
import subprocess
import sys

import numpy as np
import torch

from conftest import ROOT


def _run(extra, env_extra=None, timeout=300):
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "LOCAL_RANK", "WORLD_SIZE", "MASTER_ADDR", "MASTER_PORT")}
    env.update(env_extra or {})
    return subprocess.run([sys.executable, os.path.join(ROOT, "bench.py")] + extra, env=env, stdout=subprocess.PIPE,
                          stderr=subprocess.PIPE, timeout=timeout, cwd=ROOT)


def test_gpus_2_spawns_two_ranks_and_reports_them():
    r = _run(["--gpus", "2", "--backend", "gloo", "--steps", "3", "--warmup", "1"])
    assert r.returncode == 0, r.stderr.decode()[-2000:]
    lines = [ln for ln in r.stdout.decode().splitlines() if ln.strip()]
    assert len(lines) == 1, lines
    out = json.loads(lines[0])
    assert out["n_gpus"] == 2 and out["steps"] == 3 and out["warmup"] == 1
    assert out["stub"] is True and out["value"] is None          # not a measurement
    assert out["extra"]["allreduce_check"] is True                # the gradient all-reduce summed over both ranks


def test_more_gpus_than_devices_is_an_error_not_a_single_rank_run():
    r = _run(["--gpus", "8", "--steps", "1", "--warmup", "0"], timeout=120)
    assert r.returncode != 0
    assert b"device(s) visible" in r.stderr and r.stdout.strip() == b""


def test_steps_below_one_is_an_error():
    r = _run(["--steps", "0", "--warmup", "0"], timeout=120)
    assert r.returncode != 0 and b"--steps must be at least 1" in r.stderr and r.stdout.strip() == b""


def test_bench_inputs_are_the_same_in_every_process_and_leave_the_callers_random_state():
    """`--dump-outputs` compares two runs output for output: the inputs of make_problem (parameters, y0, t) must not depend
    on the process's global random state, and making them must not move it."""
    code = ("import hashlib, sys, torch; sys.path.insert(0, %r); import bench\n"
            "torch.manual_seed(5); a = torch.rand(3); torch.manual_seed(5)\n"
            "for wl in ('yeast', 'breast'):\n"
            "    net, y0, t = bench.make_problem(bench.WORKLOADS[wl], 'cpu', 0)\n"
            "    h = hashlib.sha256()\n"
            "    for x in list(net.parameters()) + [y0, t]:\n"
            "        h.update(x.detach().numpy().tobytes())\n"
            "    print(wl, h.hexdigest())\n"
            "print('rng', torch.equal(torch.rand(3), a))\n" % ROOT)
    outs = []
    for _ in range(2):
        r = subprocess.run([sys.executable, "-c", code], stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=300, cwd=ROOT)
        assert r.returncode == 0, r.stderr.decode()[-2000:]
        outs.append(r.stdout.decode().split())
    assert outs[0] == outs[1], outs
    assert outs[0][-2:] == ["rng", "True"], outs[0]


def _grads_on(net, y):
    torch.manual_seed(1)
    for p in net.parameters():
        p.grad = torch.randn_like(p)
    y.grad = torch.randn_like(y)


def test_dump_outputs_writes_every_array_as_float32(tmp_path):
    import bench
    import phoenix_amd
    torch.manual_seed(0)
    net = phoenix_amd.ODENet("cpu", 30, neurons=6)
    y = torch.rand(4, 1, 30, requires_grad=True)
    sol = torch.stack([y.detach(), 2 * y.detach()])
    _grads_on(net, y)
    bench.dump_outputs(str(tmp_path), sol, y, net)
    want = {"solution": sol, "grad_y0": y.grad}
    want.update({"grad_" + n.replace(".", "_"): p.grad for n, p in net.named_parameters()})
    assert sorted(f[:-4] for f in os.listdir(tmp_path)) == sorted(want) and len(want) == 8
    for name, x in want.items():
        a = np.load(str(tmp_path / (name + ".npy")))
        assert a.dtype == np.float32 and np.array_equal(a, x.numpy()), name


def test_dump_outputs_above_the_budget_keeps_the_same_seeded_sample(tmp_path, monkeypatch):
    import bench
    import phoenix_amd
    torch.manual_seed(0)
    net = phoenix_amd.ODENet("cpu", 300, neurons=20)
    y = torch.rand(16, 1, 300, requires_grad=True)
    sol = torch.stack([y.detach(), 2 * y.detach()])
    _grads_on(net, y)
    full = sum(x.numel() for x in [sol, y] + list(net.parameters())) * 4
    monkeypatch.setattr(bench, "DUMP_BYTES", full // 5)
    runs = []
    for k in range(2):
        d = tmp_path / str(k)
        bench.dump_outputs(str(d), sol, y, net)
        runs.append({f: np.load(str(d / f)) for f in os.listdir(d)})
        assert sum(os.path.getsize(str(d / f)) for f in os.listdir(d)) <= full // 5 + 128 * len(runs[-1])
    assert sorted(runs[0]) == sorted(runs[1])
    for f, a in runs[0].items():
        assert a.dtype == np.float32 and a.ndim == 1 and 0 < a.size and np.array_equal(a, runs[1][f]), f
    src = sol.numpy().reshape(-1)
    assert np.isin(runs[0]["solution.npy"], src).all()
