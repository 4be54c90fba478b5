#!/usr/bin/env python3
"""Knockout screens of the Hill simulator, phx_hill_knockouts against what a user did before it (run on the MI355X, a fresh
process):
    python tools/bench_hill_knockouts.py [--K 64 350] [--B 150] [--repeats 5] [--kpt 1 2 4 8] [--loop-launches 0]
                                         [--out profiles/hill_knockouts.json]
The shipped 350-gene network (tests/golden/g11_hill.npz), B states, times (0, 2, 3, 7, 9), dt_max = 0.01: 3 600 RHS
evaluations per trajectory.  Per K (knockouts of genes spread over the network, level 0):
    kpt_<n>              one phx_hill_knockouts call with n calls per workgroup (PHX_HILLKO_KPT; every n the kernel supports
                         at this N -- the one without the variable set is the shipped one)
    simulate_loop        K back-to-back `HillSystem.simulate` launches of the same B rows on the UNMODIFIED system: the loop
                         over K modified systems that a user ran before, minus the host work of building them -- it favours
                         the baseline, and it is k_hill_simulate, never the code under test.  The launches are identical and
                         run one after the other, so `--loop-launches L` (0: all K) times L of them and scales by K / L;
                         the JSON says how many were timed
    simulate_replicated  one `simulate` launch of the K * B replicated rows (the same work as the loop, the device filled)
Warm-up of every variant on a screen of 8 knockouts (code objects, clocks; the variants' results are compared there: bit for
bit among the group sizes, and the -1 call against `simulate`), then `--repeats` rounds (one number, or one per K) that
alternate the variants, device events around whole screens, median.  Reads nothing outside the tree; writes one JSON file,
rewritten after every K."""
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

TIMES, DT_MAX = (0.0, 2.0, 3.0, 7.0, 9.0), 0.01


def timed(fn):
    """milliseconds of one fn(), by device events around it"""
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b)


def with_kpt(n, fn):
    def run():
        os.environ["PHX_HILLKO_KPT"] = str(n)
        try:
            return fn()
        finally:
            del os.environ["PHX_HILLKO_KPT"]
    return run


def clocks():
    prop = torch.cuda.get_device_properties(0)
    out = {"compute_units": prop.multi_processor_count, "max_clock_mhz": getattr(prop, "clock_rate", 0) / 1000.0}
    try:
        out["current_clock_mhz"] = float(torch.cuda.clock_rate())
    except Exception as e:                                         # no management library in this environment
        out["current_clock_mhz"] = "not available (%s)" % type(e).__name__
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--K", type=int, nargs="+", default=[64, 350])
    ap.add_argument("--B", type=int, default=150)
    ap.add_argument("--repeats", type=int, nargs="+", default=[5])
    ap.add_argument("--loop-launches", type=int, default=0)
    ap.add_argument("--kpt", type=int, nargs="+", default=[1, 2, 4, 8])
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "hill_knockouts.json"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("bench_hill_knockouts.py measures on the GPU; none is visible")
    dev = torch.device("cuda:0")
    g = dict(np.load(os.path.join(ROOT, "tests", "golden", "g11_hill.npz")))
    system = HillSystem([str(x) for x in g["names"]], [str(x) for x in g["eqns"]], device=dev)
    N, lib = system.N, _lib.load()
    os.environ.pop("PHX_HILLKO_KPT", None)
    shipped = lib.phx_debug_hill_knockouts_kpt(N)
    kpts = []
    for n in a.kpt:                                                # every group size the kernel takes at this N
        os.environ["PHX_HILLKO_KPT"] = str(n)
        if lib.phx_debug_hill_knockouts_kpt(N) == n:
            kpts.append(n)
        del os.environ["PHX_HILLKO_KPT"]
    kpts = sorted(set(kpts) | {shipped})
    x0 = torch.from_numpy(system.sample_initial(a.B, rng=np.random.default_rng(0))).to(dev)
    res = {"network": "tests/golden/g11_hill.npz", "N": N, "B": a.B, "times": list(TIMES), "dt_max": DT_MAX,
           "rhs_evaluations_per_trajectory": 3600, "device": torch.cuda.get_device_name(0),
           "clocks_before": clocks(), "kpt_shipped": shipped, "kpt_timed": kpts,
           "library_sha256": hashlib.sha256(open(_lib.lib_path(), "rb").read()).hexdigest(), "screens": []}
    def write():
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)
            f.write("\n")

    def variants(K, launches):
        genes = [int(x) for x in np.linspace(0, N - 1, K).round()]
        reps = x0.repeat(K, 1)

        def loop():
            for _ in range(launches):
                last = system.simulate(x0, TIMES, DT_MAX)
            return last

        runs = {"kpt_%d" % n: with_kpt(n, lambda: system.knockouts(x0, TIMES, genes, 0.0, DT_MAX)) for n in kpts}
        runs["simulate_loop"] = loop
        runs["simulate_replicated"] = lambda: system.simulate(reps, TIMES, DT_MAX)
        return runs

    first = {}
    for k, f in variants(8, 2).items():                            # warm-up, and the results of the variants
        ms = timed(lambda: first.__setitem__(k, f()))
        print("warm-up %s: %.1f ms" % (k, ms), flush=True)
    ref = first["kpt_%d" % kpts[0]]
    res["variants_bitwise_equal_to_kpt_%d" % kpts[0]] = {k: bool(torch.equal(v, ref)) for k, v in first.items()
                                                          if k.startswith("kpt_")}
    free = system.knockouts(x0, TIMES, [-1], 0.0, DT_MAX)[:, 0]
    res["unperturbed_call_max_abs_diff_vs_simulate"] = float((free - first["simulate_loop"]).abs().max())
    del first, ref, free
    for i, K in enumerate(a.K):
        repeats = a.repeats[min(i, len(a.repeats) - 1)]
        launches = K if a.loop_launches <= 0 else min(K, a.loop_launches)
        runs = variants(K, launches)
        times = {k: [] for k in runs}
        for r in range(repeats):
            for k, f in runs.items():
                times[k].append(timed(f) * (K / launches if k == "simulate_loop" else 1.0))
            print("K=%d round %d: %s" % (K, r, ", ".join("%s %.1f" % (k, v[-1]) for k, v in times.items())), flush=True)
        med = {k: float(np.median(v)) for k, v in times.items()}
        best = min((k for k in runs if k.startswith("kpt_")), key=lambda k: med[k])
        row = {"K": K, "trajectories": K * a.B, "repeats": repeats, "simulate_loop_launches_timed": launches,
               "screen_ms": {k: {"median": med[k], "min": min(v), "all": v} for k, v in times.items()},
               "fastest": best, "simulate_loop_over_shipped": med["simulate_loop"] / med["kpt_%d" % shipped],
               "simulate_replicated_over_shipped": med["simulate_replicated"] / med["kpt_%d" % shipped],
               "kpt_1_over_shipped": med["kpt_1"] / med["kpt_%d" % shipped] if "kpt_1" in med else None}
        res["screens"].append(row)
        res["clocks_after"] = clocks()
        write()
        print("K=%d: %s; fastest %s; simulate loop / shipped (kpt %d) = %.2f x, replicated rows / shipped = %.2f x"
              % (K, ", ".join("%s %.1f ms" % (k, med[k]) for k in runs), best, shipped, row["simulate_loop_over_shipped"],
                 row["simulate_replicated_over_shipped"]), flush=True)


if __name__ == "__main__":
    main()
