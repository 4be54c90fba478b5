#!/usr/bin/env python3
"""Pair knockouts of the Hill simulator, and what the set test of phx_hill_knockout_sets costs (run on the MI355X, a fresh
process):
    python tools/bench_hill_knockout_pairs.py [--genes 16] [--B 150] [--repeats 3] [--out profiles/hill_knockout_pairs.json]
The shipped 350-gene network (tests/golden/g11_hill.npz), B states, times (0, 2, 3, 7, 9), dt_max = 0.01, G genes spread over
the network at level 0 and all their K = G (G - 1) / 2 pairs (16 genes: 120 pairs):
    knockout_pairs       `HillSystem.knockout_pairs`, the whole screen: the -1 call, the G single calls, the K pair calls in
                         blocks of 64, the scoring passes, the scores copied to the host
    pair_calls           the K pair calls alone, one `HillSystem.knockouts` pass at width 2
    single_entry         K single-gene calls (the first gene of every pair) through phx_hill_knockouts
    single_sets_w<W>     the same K calls as sets through phx_hill_knockout_sets, their rows padded with -1 to W = 1, 2, 4
                         entries: W = 1 is the single-gene kernel itself, W = 2 and 4 run the same arithmetic behind the
                         W-entry clamp test -- what that test costs, and what fewer calls per launch cost (256 / W)
Warm-up of every variant on the pairs of 4 genes (code objects, clocks; the single-call variants are compared there, bit for
bit), then `--repeats` rounds that alternate the variants, device events around whole screens, median.  There is no
threshold here, only recorded numbers.  Reads nothing outside the tree; writes one JSON file."""
import argparse
import ctypes as C
import hashlib
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from phoenix_amd import _lib, engine                               # noqa: E402
from phoenix_amd.simulator import HillSystem                       # noqa: E402
from bench_hill_knockouts import DT_MAX, TIMES, clocks, timed      # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--genes", type=int, default=16)
    ap.add_argument("--B", type=int, default=150)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "hill_knockout_pairs.json"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("bench_hill_knockout_pairs.py measures on the GPU; none is visible")
    dev = torch.device("cuda:0")
    g = dict(np.load(os.path.join(ROOT, "tests", "golden", "g11_hill.npz")))
    system = HillSystem([str(x) for x in g["names"]], [str(x) for x in g["eqns"]], device=dev)
    N, lib = system.N, _lib.load()
    os.environ.pop("PHX_HILLKO_KPT", None)
    x0 = torch.from_numpy(system.sample_initial(a.B, rng=np.random.default_rng(0))).to(dev)
    t_dev = torch.tensor(TIMES, dtype=torch.float64, device=dev)

    def sets_call(rows, width):
        """phx_hill_knockout_sets on rows of `width` entries, level 0 throughout"""
        K = len(rows)
        flat = [x for r in rows for x in tuple(r) + (-1,) * (width - len(r))]
        out = torch.empty((len(TIMES), K * a.B, N), dtype=torch.float32, device=dev)
        engine._check_call(lib.phx_hill_knockout_sets(*system._args(), engine._p(x0), engine._p(t_dev), len(TIMES),
                                                      C.c_double(DT_MAX), (C.c_int * len(flat))(*flat),
                                                      (C.c_float * len(flat))(*([0.0] * len(flat))), width, K, engine._p(out),
                                                      a.B, N, engine._stream_ptr()))
        return out

    def variants(G):
        genes = [int(x) for x in np.linspace(0, N - 1, G).round()]
        pairs = [(genes[i], genes[j]) for i in range(G) for j in range(i + 1, G)]
        firsts = [p[0] for p in pairs]
        runs = {"knockout_pairs": lambda: system.knockout_pairs(x0, genes=genes, value=0.0, times=TIMES, dt_max=DT_MAX),
                "pair_calls": lambda: system.knockouts(x0, TIMES, pairs, 0.0, DT_MAX),
                "single_entry": lambda: system.knockouts(x0, TIMES, firsts, 0.0, DT_MAX).reshape(len(TIMES), -1, N)}
        for w in (1, 2, 4):
            runs["single_sets_w%d" % w] = lambda w=w: sets_call([(f,) for f in firsts], w)
        return genes, pairs, runs

    res = {"network": "tests/golden/g11_hill.npz", "N": N, "B": a.B, "times": list(TIMES), "dt_max": DT_MAX,
           "device": torch.cuda.get_device_name(0), "clocks_before": clocks(), "kpt": lib.phx_debug_hill_knockouts_kpt(N),
           "library_sha256": hashlib.sha256(open(_lib.lib_path(), "rb").read()).hexdigest()}
    first = {}
    for k, f in variants(4)[2].items():                            # warm-up, and the results of the single-call variants
        ms = timed(lambda: first.__setitem__(k, f()))
        print("warm-up %s: %.1f ms" % (k, ms), flush=True)
    res["single_sets_bitwise_equal_to_single_entry"] = {k: bool(torch.equal(v, first["single_entry"]))
                                                        for k, v in first.items() if k.startswith("single_sets")}
    del first
    genes, pairs, runs = variants(a.genes)
    times = {k: [] for k in runs}
    for r in range(a.repeats):
        for k, f in runs.items():
            times[k].append(timed(f))
        print("round %d: %s" % (r, ", ".join("%s %.1f" % (k, v[-1]) for k, v in times.items())), flush=True)
    med = {k: float(np.median(v)) for k, v in times.items()}
    res.update({"genes": genes, "pairs": len(pairs), "calls_of_the_whole_screen": 1 + len(genes) + len(pairs),
                "repeats": a.repeats, "screen_ms": {k: {"median": med[k], "min": min(v), "all": v} for k, v in times.items()},
                "single_sets_over_single_entry": {k: med[k] / med["single_entry"] for k in med if k.startswith("single_sets")},
                "pair_calls_over_single_entry": med["pair_calls"] / med["single_entry"], "clocks_after": clocks()})
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print("; ".join("%s %.1f ms" % (k, med[k]) for k in runs), flush=True)


if __name__ == "__main__":
    main()
