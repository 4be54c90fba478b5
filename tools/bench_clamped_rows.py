#!/usr/bin/env python3
"""A training step on perturbation time courses: the per-row clamp kernels against the same step unclamped and against the
grouped path (run on the MI355X):
    python tools/bench_clamped_rows.py [--shape 11165,40,60] [--sets 8] [--rounds 5] [--steps 20] [--warmup 5]
                                       [--parent-lib <libphoenix_hip.so of the parent commit>]
                                       [--out profiles/clamped_rows.json]
The step is forward + backward of `odeint_adjoint` (dopri5, per-sample grids of the breast-cancer pseudotime interval) on
B rows of which `--sets` carry one held gene each (8 distinct single-gene sets) and the rest are unperturbed.  Measured:
  clamped    clamp=<the list>: one launch of the CLAMP forms per direction;
  unclamped  the same step with clamp=None on this library -- and, with --parent-lib, on the PARENT's library in a process
             of its own (PHX_DIAG=1 PHX_LIB): the cost of the mask;
  grouped    the same list with the kernels switched off: what a user had to do before (per distinct set a cloned,
             zeroed multiplier vector and the ordinary entry points).
Every measurement is a device-synchronised window of `--steps` steps after `--warmup` steps; the ways alternate inside a
round and the rounds alternate the libraries (each worker is a fresh child process).  Reports median, min and max over the
rounds.  Reads nothing outside the tree but the library --parent-lib names; writes one JSON file."""
import argparse
import hashlib
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def worker(a):
    import numpy as np
    import torch
    import phoenix_amd as pa
    from phoenix_amd import engine
    N, H, B = (int(x) for x in a.shape.split(","))
    dev = torch.device("cuda:0")
    torch.manual_seed(0)
    net = pa.ODENet(dev, N, neurons=H)
    with torch.no_grad():
        for lin in (net.net_sums.linear_out, net.net_prods.linear_out, net.net_alpha_combine.linear_out):
            lin.weight.normal_(0.0, 0.05)
    rs = np.random.RandomState(1)
    y0 = torch.from_numpy(np.clip(rs.randn(B, 1, N) * 0.15 + 0.5, 0.03, 1.07).astype(np.float32)).to(dev)
    t = torch.tensor([[0.0, 0.0051]] * B, device=dev)
    G = torch.from_numpy((rs.randn(2, B, 1, N) * (2.0 / (B * N))).astype(np.float32)).to(dev)
    genes = [int(g) for g in np.linspace(0, N - 1, a.sets).astype(int)]
    clamp = [genes[b] if b < a.sets else -1 for b in range(B)]

    def step(cl):
        for p in net.parameters():
            p.grad = None
        y = y0.detach().requires_grad_(True)
        (pa.odeint_adjoint(net, y, t, method="dopri5", clamp=cl) * G).sum().backward()

    def window(fn):
        for _ in range(a.warmup):
            fn()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(a.steps):
            fn()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3 / a.steps

    exists = engine.clamped_rows_plan_exists

    def grouped():
        engine.clamped_rows_plan_exists = lambda *x, **k: 0
        try:
            step(clamp)
        finally:
            engine.clamped_rows_plan_exists = exists

    ways = {"unclamped": lambda: step(None)}
    if a.worker == "this":
        ways.update({"clamped": lambda: step(clamp), "grouped": grouped})
    print(json.dumps({k: window(f) for k, f in ways.items()}))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shape", default="11165,40,60")
    ap.add_argument("--sets", type=int, default=8)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--parent-lib", default=None)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "clamped_rows.json"))
    ap.add_argument("--worker", choices=("this", "parent"), default=None)
    a = ap.parse_args()
    if a.worker:
        return worker(a)
    from phoenix_amd import _lib
    args = [sys.executable, os.path.abspath(__file__), "--shape", a.shape, "--sets", str(a.sets), "--steps", str(a.steps),
            "--warmup", str(a.warmup)]
    runs = {}
    for _ in range(a.rounds):
        for who in ("this", "parent") if a.parent_lib else ("this",):
            env = dict(os.environ)
            if who == "parent":
                env.update({"PHX_DIAG": "1", "PHX_LIB": os.path.abspath(a.parent_lib)})
            out = subprocess.run(args + ["--worker", who], env=env, check=True, capture_output=True, text=True, timeout=600).stdout
            for k, v in json.loads(out.strip().splitlines()[-1]).items():
                runs.setdefault(k if who == "this" else "unclamped_parent_library", []).append(v)
    import numpy as np
    res = {"shape": a.shape, "held_rows": a.sets, "rounds": a.rounds, "steps_per_window": a.steps, "warmup": a.warmup,
           "library_sha256": hashlib.sha256(open(_lib.lib_path(), "rb").read()).hexdigest(),
           "parent_library_sha256": hashlib.sha256(open(a.parent_lib, "rb").read()).hexdigest() if a.parent_lib else None,
           "step_ms": {k: {"median": float(np.median(v)), "min": min(v), "max": max(v), "all": v} for k, v in runs.items()}}
    for k, v in res["step_ms"].items():
        print("%-26s median %.3f ms (min %.3f, max %.3f)" % (k, v["median"], v["min"], v["max"]), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
