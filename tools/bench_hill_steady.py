#!/usr/bin/env python3
"""Where the Hill simulator settles under a knockout: phx_hill_steady against the dense route and against the integration a
user ran before it (run on the MI355X, a fresh process):
    python tools/bench_hill_steady.py [--K 64 350] [--B 150] [--repeats 5] [--dense-repeats 5] [--tol 1e-5] [--t-max 60]
                                      [--out profiles/hill_steady.json]
The shipped 350-gene network (tests/golden/g11_hill.npz), B states of sample_initial(seed 0).  Per K (knockouts of genes spread
over the network, level 0):
    blocks      `HillSystem.knockout_steady_states(method="blocks")`: the baseline solve and the K * B knockout rows
    dense       the same with method="dense"
    integrate   the route that existed before: `HillSystem.knockouts` at dt_max = 0.01 from 0 to T, T the first whole time at
                which max |rate| over the genes that are not held is <= tol in EVERY row of the screen.  The script finds T
                first (blocks of 64 knockouts to whole times 0 .. t-max, `rhs` at every time); the timed call asks for the
                states at (0, T) only.  Its rows start from x0, not from the settled baseline: that is what a user had.
Warm-up of every variant on a screen of 8 knockouts, then `--repeats` rounds that alternate the variants, device events
around whole screens, a synchronisation before each; median, min and max.  `--dense-repeats` times the dense route in the
first rounds only (a whole-genome screen takes it minutes; the JSON says how many runs each figure rests on).  The settled
states of the three variants are compared.  Reads nothing outside the tree; writes one JSON file, rewritten after every K."""
import argparse
import hashlib
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from phoenix_amd import _lib                                       # noqa: E402
from phoenix_amd.simulator import HillSystem                       # noqa: E402

DT_MAX = 0.01


def timed(fn):
    """milliseconds of one fn(), by device events around it"""
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b)


def settling_time(system, x0, genes, tol, t_max):
    """the first whole T at which every row of the screen has max |rate| <= tol over the genes that are not held"""
    times = np.arange(0, t_max + 1, dtype=np.float64)
    worst = np.zeros(len(times))
    for k0 in range(0, len(genes), 64):
        part = genes[k0:k0 + 64]
        sol = system.knockouts(x0, times, part, 0.0, DT_MAX)                       # [T, k, B, N]
        rate = system.rhs(sol.reshape(-1, system.N)).reshape(sol.shape).abs()
        for i, g in enumerate(part):
            rate[:, i, :, g] = 0
        worst = np.maximum(worst, rate.amax(dim=(1, 2, 3)).cpu().numpy())
        del sol, rate
    below = np.flatnonzero(worst <= tol)
    return (int(times[below[0]]) if len(below) else None), worst.tolist()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--K", type=int, nargs="+", default=[64, 350])
    ap.add_argument("--B", type=int, default=150)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--dense-repeats", type=int, default=None)
    ap.add_argument("--tol", type=float, default=1e-5)
    ap.add_argument("--t-max", type=int, default=60)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "hill_steady.json"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("bench_hill_steady.py measures on the GPU; none is visible")
    dev = torch.device("cuda:0")
    g = dict(np.load(os.path.join(ROOT, "tests", "golden", "g11_hill.npz")))
    system = HillSystem([str(x) for x in g["names"]], [str(x) for x in g["eqns"]], device=dev)
    N = system.N
    x0 = torch.from_numpy(system.sample_initial(a.B, rng=np.random.default_rng(0))).to(dev)
    blk = system.block_structure()
    res = {"network": "tests/golden/g11_hill.npz", "N": N, "B": a.B, "tol": a.tol, "dt_max": DT_MAX,
           "components": len(blk.comp_ptr) - 1, "levels": len(blk.level_ptr) - 1, "largest_component": blk.largest,
           "device": torch.cuda.get_device_name(0), "compute_units": torch.cuda.get_device_properties(0).multi_processor_count,
           "library_sha256": hashlib.sha256(open(_lib.lib_path(), "rb").read()).hexdigest(), "screens": []}

    def write():
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)
            f.write("\n")

    def variants(genes, T):
        return {"blocks": lambda: system.knockout_steady_states(x0, genes, 0.0, tol=a.tol, method="blocks"),
                "dense": lambda: system.knockout_steady_states(x0, genes, 0.0, tol=a.tol, method="dense"),
                "integrate": lambda: system.knockouts(x0, [0.0, float(T)], genes, 0.0, DT_MAX)}

    for k, f in variants([int(x) for x in np.linspace(0, N - 1, 8).round()], 2).items():      # code objects, clocks
        print("warm-up %s: %.1f ms" % (k, timed(f)), flush=True)
    for K in a.K:
        genes = [int(x) for x in np.linspace(0, N - 1, K).round()]
        T, worst = settling_time(system, x0, genes, a.tol, a.t_max)
        print("K=%d: every row below tol at T = %s" % (K, T), flush=True)
        row = {"K": K, "rows": K * a.B, "repeats": a.repeats, "integrate_T": T, "integrate_rhs_evaluations_per_row":
               None if T is None else int(round(4 * T / DT_MAX)), "max_rate_at_whole_times": worst}
        if T is None:
            row["integrate"] = "not measured: no whole T <= %d brings every row below tol" % a.t_max
        runs = {k: f for k, f in variants(genes, T or 1).items() if k != "integrate" or T is not None}
        times, last = {k: [] for k in runs}, {}
        dense_repeats = a.repeats if a.dense_repeats is None else max(1, min(a.repeats, a.dense_repeats))
        for r in range(a.repeats):
            for k, f in runs.items():
                if k == "dense" and r >= dense_repeats:
                    continue
                times[k].append(timed(lambda: last.__setitem__(k, f())))
            print("K=%d round %d: %s" % (K, r, ", ".join("%s %.1f ms" % (k, v[-1]) for k, v in times.items())), flush=True)
        row["screen_ms"] = {k: {"median": float(np.median(v)), "min": min(v), "max": max(v), "runs": len(v), "all": v}
                            for k, v in times.items()}
        med = {k: row["screen_ms"][k]["median"] for k in runs}
        yb = last["blocks"].knockouts.y.reshape(K, a.B, N)
        row["status_not_0"] = {k: int((last[k].knockouts.status != 0).sum()) + int((last[k].base.status != 0).sum())
                               for k in ("blocks", "dense")}
        row["steps_blocks"] = {"max": int(last["blocks"].knockouts.iterations.max()),
                               "mean": float(last["blocks"].knockouts.iterations.float().mean())}
        row["max_abs_diff_dense_vs_blocks"] = float((last["dense"].knockouts.y.reshape(K, a.B, N) - yb).abs().max())
        row["dense_over_blocks"] = med["dense"] / med["blocks"]
        if T is not None:
            row["max_abs_diff_integrate_vs_blocks"] = float((last["integrate"][-1] - yb).abs().max())
            row["integrate_over_blocks"] = med["integrate"] / med["blocks"]
        res["screens"].append(row)
        write()
        print("K=%d: %s" % (K, ", ".join("%s %.1f ms (%.1f .. %.1f)" % (k, med[k], min(times[k]), max(times[k])) for k in runs)),
              flush=True)
        last.clear()


if __name__ == "__main__":
    main()
