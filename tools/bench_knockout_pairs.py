#!/usr/bin/env python3
"""Pair knockout screen, clamped launches against the host loop it replaces (run on the MI355X, a fresh process):
    python tools/bench_knockout_pairs.py [--genes 16] [--T 10] [--repeats 5] [--shapes 11165,40,60 14691,200,24]
                                         [--out profiles/knockout_pairs.json]
Per shape (N, H, B): `knockout_pairs` over all pairs of `--genes` genes (dopri5, T outputs, value 0) at pairs_per_launch 1
and 8, and the same screen as the host loop a user had before -- the baseline, per gene and per pair one `odeint` on a
module whose gene_multipliers entries are zeroed (a parameter re-layout and one launch each), scored by torch ops --
alternating the three.  Warm-up, HIP events around whole screens, median of the repeats.  Reads nothing outside the tree;
writes one JSON file."""
import argparse
import hashlib
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import phoenix_amd as pa                                           # noqa: E402
from phoenix_amd import _lib                                       # noqa: E402


def timed(fn):
    """milliseconds of one fn(), by device events around it"""
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b)


def host_loop(net, znet, y0, genes, t):
    """the screen without the sets: per single and per pair zeroed multipliers on a copy, one solve, torch scoring ->
    (scores [K], interaction_scores [K]) over all pairs of `genes`"""
    N = y0.shape[-1]
    pairs = [(i, j) for i in range(len(genes)) for j in range(i + 1, len(genes))]
    scores = torch.empty(len(pairs), dtype=torch.float32, device=y0.device)
    iscores = torch.empty(len(pairs), dtype=torch.float32, device=y0.device)

    def held(idx):
        znet.gene_multipliers.copy_(net.gene_multipliers)
        y0k = y0.clone()
        for g in idx:
            znet.gene_multipliers.reshape(-1)[g] = 0.0
            y0k[:, 0, g] = 0.0
        return pa.odeint(znet, y0k, t, method="dopri5")

    with torch.no_grad():
        base = pa.odeint(net, y0, t, method="dopri5")
        d1 = [(held([g]) - base)[1:] for g in genes]
        for k, (i, j) in enumerate(pairs):
            dab = (held([genes[i], genes[j]]) - base)[1:]
            keep = torch.ones(N, dtype=torch.bool, device=y0.device)
            keep[[genes[i], genes[j]]] = False
            scores[k] = dab.abs().mean(dim=(0, 1, 2))[keep].mean()
            iscores[k] = (dab - (d1[i] + d1[j])).abs().mean(dim=(0, 1, 2))[keep].mean()
    return scores.cpu().numpy(), iscores.cpu().numpy()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--genes", type=int, default=16)
    ap.add_argument("--T", type=int, default=10)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--shapes", nargs="+", default=["11165,40,60", "14691,200,24"])
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "knockout_pairs.json"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("bench_knockout_pairs.py measures on the GPU; none is visible")
    dev = torch.device("cuda:0")
    res = {"genes": a.genes, "pairs": a.genes * (a.genes - 1) // 2, "outputs": a.T, "method": "dopri5", "repeats": a.repeats,
           "device": torch.cuda.get_device_name(0),
           "library_sha256": hashlib.sha256(open(_lib.lib_path(), "rb").read()).hexdigest(), "shapes": []}
    t = torch.from_numpy(np.arange(a.T) / a.T).to(dev)
    for shape in a.shapes:
        N, H, B = (int(x) for x in shape.split(","))
        torch.manual_seed(0)
        net, znet = pa.ODENet(dev, N, neurons=H), pa.ODENet(dev, N, neurons=H)
        with torch.no_grad():
            for prm in net.parameters():
                prm.mul_(0.5)
            for q, prm in zip(znet.parameters(), net.parameters()):
                q.copy_(prm)
        genes = list(range(0, N, max(1, N // a.genes)))[:a.genes]
        y0 = torch.rand(B, 1, N, device=dev) - 0.5

        def screen(per_launch):
            r = pa.knockout_pairs(net, y0, genes=genes, time_pts_to_project=t, pairs_per_launch=per_launch, want_matrices=False)
            return r.scores, r.interaction_scores

        runs = {"sets_1": lambda: screen(1), "sets_8": lambda: screen(8), "host_loop": lambda: host_loop(net, znet, y0, genes, t)}
        first = {k: f() for k, f in runs.items()}                  # warm-up, and the scores of the three ways
        times = {k: [] for k in runs}
        for _ in range(a.repeats):
            for k, f in runs.items():
                times[k].append(timed(f))
        med = {k: float(np.median(v)) for k, v in times.items()}
        row = {"N": N, "H": H, "B": B, "calls_per_launch_of_8": _lib.load().phx_debug_calls_grids_plan(
                   N, H, B * 8, a.T, 8, _lib.METHODS["dopri5"], None),
               "screen_ms": {k: {"median": med[k], "min": min(times[k]), "all": times[k]} for k in runs},
               "host_loop_over_sets_8": med["host_loop"] / med["sets_8"],
               "host_loop_over_sets_1": med["host_loop"] / med["sets_1"],
               "scores_max_rel_diff_vs_host_loop": float(np.max(np.abs(first["sets_8"][0] - first["host_loop"][0]) /
                                                                np.abs(first["host_loop"][0]))),
               "interaction_scores_max_diff_vs_host_loop_over_max_score": float(
                   np.max(np.abs(first["sets_8"][1] - first["host_loop"][1])) / np.max(np.abs(first["host_loop"][0])))}
        res["shapes"].append(row)
        print("N=%d H=%d B=%d, %d pairs of %d genes: sets x8 %.1f ms, sets x1 %.1f ms, host loop %.1f ms (%.2f x / %.2f x)" %
              (N, H, B, res["pairs"], len(genes), med["sets_8"], med["sets_1"], med["host_loop"], row["host_loop_over_sets_8"],
               row["host_loop_over_sets_1"]), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
