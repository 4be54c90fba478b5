#!/usr/bin/env python3
"""Knockout screen, clamped launches against the host loop it replaces (run on the MI355X, a fresh process):
    python tools/bench_knockout.py [--genes 64] [--T 10] [--repeats 5] [--shapes 11165,40,60 14691,200,24]
                                   [--out profiles/knockout_scan.json]
Per shape (N, H, B): `knockout_effects` over `--genes` genes (dopri5, T outputs, value 0) at genes_per_launch 1 and 8, and
the same knockouts as a host loop -- per gene one `odeint` on a module whose gene_multipliers entry is zeroed (a parameter
re-layout and one launch per gene), scored by torch ops -- alternating the three.  Warm-up, HIP events around whole
screens, median of the repeats.  Reads nothing outside the tree; writes one JSON file."""
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
    """the screen without the clamp: per gene a zeroed multiplier, one solve, torch scoring -> scores [G]"""
    N = y0.shape[-1]
    scores = torch.empty(len(genes), dtype=torch.float32, device=y0.device)
    with torch.no_grad():
        base = pa.odeint(net, y0, t, method="dopri5")
        for i, g in enumerate(genes):
            znet.gene_multipliers.copy_(net.gene_multipliers)
            znet.gene_multipliers.reshape(-1)[g] = 0.0
            y0k = y0.clone()
            y0k[:, 0, g] = 0.0
            mag = (pa.odeint(znet, y0k, t, method="dopri5") - base)[1:].abs().mean(dim=(0, 1, 2))
            scores[i] = (mag.sum() - mag[g]) / (N - 1)
    return scores.cpu().numpy()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--genes", type=int, default=64)
    ap.add_argument("--T", type=int, default=10)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--shapes", nargs="+", default=["11165,40,60", "14691,200,24"])
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "knockout_scan.json"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("bench_knockout.py measures on the GPU; none is visible")
    dev = torch.device("cuda:0")
    res = {"genes": a.genes, "outputs": a.T, "method": "dopri5", "repeats": a.repeats, "device": torch.cuda.get_device_name(0),
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
        runs = {"clamped_1": lambda: pa.knockout_effects(net, y0, genes=genes, time_pts_to_project=t, genes_per_launch=1,
                                                         want_matrices=False).scores,
                "clamped_8": lambda: pa.knockout_effects(net, y0, genes=genes, time_pts_to_project=t, genes_per_launch=8,
                                                         want_matrices=False).scores,
                "host_loop": lambda: host_loop(net, znet, y0, genes, t)}
        first = {k: f() for k, f in runs.items()}                  # warm-up, and the scores of the three ways
        times = {k: [] for k in runs}
        for _ in range(a.repeats):
            for k, f in runs.items():
                times[k].append(timed(f))
        med = {k: float(np.median(v)) for k, v in times.items()}
        row = {"N": N, "H": H, "B": B, "calls_per_launch_of_8": _lib.load().phx_debug_calls_grids_plan(
                   N, H, B * 8, a.T, 8, _lib.METHODS["dopri5"], None),
               "screen_ms": {k: {"median": med[k], "min": min(times[k]), "all": times[k]} for k in runs},
               "host_loop_over_clamped_8": med["host_loop"] / med["clamped_8"],
               "host_loop_over_clamped_1": med["host_loop"] / med["clamped_1"],
               "scores_max_rel_diff_vs_host_loop": float(np.max(np.abs(first["clamped_8"] - first["host_loop"]) /
                                                                np.abs(first["host_loop"])))}
        res["shapes"].append(row)
        print("N=%d H=%d B=%d, %d knockouts: clamped x8 %.1f ms, clamped x1 %.1f ms, host loop %.1f ms (%.2f x / %.2f x)" %
              (N, H, B, len(genes), med["clamped_8"], med["clamped_1"], med["host_loop"], row["host_loop_over_clamped_8"],
               row["host_loop_over_clamped_1"]), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
