#!/usr/bin/env python3
"""Gene-influence scan, eager scoring against the fused scoring pass (run on the MI355X):
    python tools/bench_influence.py [--genes 16] [--N 11165] [--H 40] [--n 60] [--per-launch 8] [--repeats 10]
                                    [--out profiles/influence_scan.json]
Times a scan of `--genes` genes (dopri5, 10 outputs) with gene_influence_scores(fused=False) -- the code path the scan
had before the scoring kernel -- and with fused=True, alternating the two; then the scoring kernel alone on one launch's
output block, and a plain device-to-device copy of the bytes that kernel reads, as the yardstick of what this device
streams.  Warm-up, HIP events, median of the repeats.  Reads nothing outside the tree; writes one JSON file."""
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
from phoenix_amd import _lib, engine                               # noqa: E402

HBM_PEAK = 8.0e12      # bytes/s, the device's specified peak


def timed(fn, repeats, warmup=2):
    """milliseconds of every repeat of fn(), by device events around it"""
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    out = []
    for _ in range(repeats):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        out.append(a.elapsed_time(b))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--genes", type=int, default=16)
    ap.add_argument("--N", type=int, default=11165)
    ap.add_argument("--H", type=int, default=40)
    ap.add_argument("--n", type=int, default=60)
    ap.add_argument("--per-launch", type=int, default=8)
    ap.add_argument("--repeats", type=int, default=10)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "influence_scan.json"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("bench_influence.py measures on the GPU; none is visible")
    dev = torch.device("cuda:0")
    N, k, n, T = a.N, a.per_launch, a.n, 10
    torch.manual_seed(0)
    net = pa.ODENet(dev, N, neurons=a.H)
    with torch.no_grad():
        for prm in net.parameters():
            prm.mul_(0.5)
    genes = list(range(0, N, max(1, N // a.genes)))[:a.genes]
    kw = dict(n_random_inputs_per_gene=n, device=dev, genes=genes, genes_per_launch=k)
    res = {"shape": {"N": N, "H": a.H, "n": n, "outputs": T, "genes": len(genes), "genes_per_launch": k, "method": "dopri5"},
           "repeats": a.repeats, "device": torch.cuda.get_device_name(0),
           "library_sha256": hashlib.sha256(open(_lib.lib_path(), "rb").read()).hexdigest()}

    # the scan, both ways, alternating (the same seed in front of every scan: the same draws, the same solves)
    def scan(fused):
        torch.manual_seed(1)
        return pa.gene_influence_scores(net, N, "dopri5", fused=fused, **kw)

    s_eager, s_fused = scan(False), scan(True)
    res["scores_max_rel_diff"] = float(np.max(np.abs(s_fused - s_eager) / np.abs(s_eager)))
    times = {False: [], True: []}
    for _ in range(a.repeats):
        for fused in (False, True):
            times[fused] += timed(lambda: scan(fused), 1, warmup=0)
    res["scan_ms"] = {"eager": {"median": float(np.median(times[False])), "min": min(times[False]), "all": times[False]},
                      "fused": {"median": float(np.median(times[True])), "min": min(times[True]), "all": times[True]}}
    res["scan_speedup_median"] = res["scan_ms"]["eager"]["median"] / res["scan_ms"]["fused"]["median"]

    # the scoring kernel alone on one launch's block, against a copy of the bytes it reads
    torch.manual_seed(2)
    sol = torch.rand((T, 2 * k * n, N), device=dev)
    read_bytes = (T - 1) * 2 * k * n * N * 4                       # every output but the first, once
    launch_genes = genes[:k]
    dst = torch.empty_like(sol[1:])
    t_kernel = timed(lambda: engine.influence_scores(sol, k, n, launch_genes), max(a.repeats, 20), warmup=5)
    t_matrix = timed(lambda: engine.influence_scores(sol, k, n, launch_genes, want_targets=True), max(a.repeats, 20), warmup=5)
    t_copy = timed(lambda: dst.copy_(sol[1:]), max(a.repeats, 20), warmup=5)
    # the eager scoring tail of the same block (the per-gene torch ops of analysis.influence_score)
    out = sol.reshape((T, 2 * k, n, 1, N)).transpose(0, 1)

    def eager_tail():
        sc = torch.zeros(k, dtype=torch.float32, device=dev)
        for j, g in enumerate(launch_genes):
            sc[j] = pa.analysis.influence_score(out[2 * j], out[2 * j + 1], g)
        return sc

    t_tail = timed(eager_tail, max(a.repeats, 20), warmup=5)
    med = lambda v: float(np.median(v))                            # noqa: E731
    bw = read_bytes / (med(t_kernel) * 1e-3)
    # a copy moves its bytes twice (read + write); its READ rate is the like-for-like figure
    copy_read_bw = read_bytes / (med(t_copy) * 1e-3)
    res["kernel"] = {"block_bytes_read": read_bytes, "scores_only_ms": med(t_kernel), "with_targets_ms": med(t_matrix),
                     "eager_tail_ms": med(t_tail), "read_bandwidth_bytes_per_s": bw, "fraction_of_hbm_peak": bw / HBM_PEAK,
                     "copy_same_bytes_ms": med(t_copy), "copy_read_bytes_per_s": copy_read_bw,
                     "copy_moved_bytes_per_s": 2 * copy_read_bw, "kernel_time_over_copy_time": med(t_kernel) / med(t_copy)}
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps({k_: v for k_, v in res.items() if k_ != "scan_ms"}))
    print("scan of %d genes: eager %.2f ms, fused %.2f ms (median of %d); scoring kernel %.3f ms = %.2f TB/s = %.0f %% of "
          "the 8 TB/s peak; copy of the same bytes %.3f ms" %
          (len(genes), res["scan_ms"]["eager"]["median"], res["scan_ms"]["fused"]["median"], a.repeats, med(t_kernel),
           bw / 1e12, 100 * bw / HBM_PEAK, med(t_copy)))


if __name__ == "__main__":
    main()
