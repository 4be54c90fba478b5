#!/usr/bin/env python3
"""Pathway permutation tests, `pathway_permutation_test` against the torch formulation on the same GPU (run on the MI355X):
    python tools/bench_pathways.py [--N 11165] [--P 7000] [--R 500,100000] [--repeats 5] [--out profiles/pathway_permutation.json]
The problem: N genes with random scores, P pathways whose sizes are drawn log-uniform in [10, 500].  Per R:
  - `pathway_permutation_test` as a whole (the checks and the size ordering of the pathways included), and the kernel call
    alone on prepared device arrays;
  - the kernel call with PHX_DIAG=1 PHX_PATHWAYS_STAGES=1 | 2 | 3 (every permutation ends after its keys, its sort, its score
    image): the differences are the stages' shares, and members x R x 4 bytes over the walk's share is the achieved LDS
    gather rate;
  - the torch formulation in chunks of permutations that fit memory: `torch.rand(Rc, N).argsort()`, a gather of the scores,
    then the membership product as a dense float32 matmul and as `torch.sparse.mm`, and the same count / s1 / s2
    reductions.  It is timed over at most --torch-perms permutations and scaled to R (the dense product at R = 10^5 is
    1.6 x 10^13 operations); the JSON says how many were run.
Warm-up, HIP events, median of the repeats; the clocks `rocm-smi --showclocks` reports before and after are recorded when
the command exists.  Reads nothing outside the tree; writes one JSON file."""
import argparse
import hashlib
import json
import os
import subprocess
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import phoenix_amd as pa                                           # noqa: E402
from phoenix_amd import _lib, engine                               # noqa: E402
from tools.bench_effects import timed                              # noqa: E402

STAGES = ("keys", "sort", "image", "walk")


def clocks():
    try:
        out = subprocess.run(["rocm-smi", "--showclocks", "-d", "0"], capture_output=True, text=True, timeout=30).stdout
        return [line.strip() for line in out.splitlines() if "clk" in line.lower()] or "no clock lines"
    except (OSError, subprocess.SubprocessError) as e:
        return "unavailable (%s)" % type(e).__name__


def problem(N, P, seed=0):
    rng = np.random.default_rng(seed)
    sizes = np.minimum(N, np.exp(rng.uniform(np.log(10), np.log(500), P)).astype(np.int64))
    ptr = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)
    idx = np.concatenate([rng.choice(N, m, replace=False) for m in sizes]).astype(np.int32)
    return rng.random(N).astype(np.float32), ptr, idx


def torch_form(scores, member, base, R, chunk, sparse):
    """count, s1, s2 of R fresh permutations: member is [P, N] float32, dense or sparse CSR"""
    P, N = member.shape
    count = torch.zeros(P, dtype=torch.int64, device=scores.device)
    s1 = torch.zeros(P, dtype=torch.float64, device=scores.device)
    s2 = torch.zeros(P, dtype=torch.float64, device=scores.device)
    for r0 in range(0, R, chunk):
        rc = min(chunk, R - r0)
        order = torch.rand((rc, N), device=scores.device).argsort(dim=1)
        permuted = scores[order]                                                   # [Rc, N]
        x = torch.sparse.mm(member, permuted.t()).t() if sparse else permuted @ member.t()     # [Rc, P]
        d = x.to(torch.float64) - base
        count += (d > 0).sum(0)
        s1 += d.sum(0)
        s2 += (d * d).sum(0)
    return count, s1, s2


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--N", type=int, default=11165)
    ap.add_argument("--P", type=int, default=7000)
    ap.add_argument("--R", default="500,100000")
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--chunk", type=int, default=2048, help="permutations of a chunk of the torch formulation")
    ap.add_argument("--torch-perms", type=int, default=4096, help="permutations the torch formulation is timed over at most")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "pathway_permutation.json"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("bench_pathways.py measures on the GPU; none is visible")
    dev = torch.device("cuda:0")
    med = lambda v: float(np.median(v))                            # noqa: E731
    scores, ptr, idx = problem(a.N, a.P)
    pw = pa.Pathways(["p%d" % k for k in range(a.P)], ptr, idx, np.arange(a.N))
    nnz = int(ptr[-1])
    s_d, ptr_d, idx_d = (torch.from_numpy(x).to(dev) for x in (scores, ptr, idx))
    owner = torch.repeat_interleave(torch.arange(a.P, device=dev), ptr_d[1:] - ptr_d[:-1])
    dense = torch.zeros((a.P, a.N), dtype=torch.float32, device=dev)
    dense[owner, idx_d.long()] = 1
    csr = dense.to_sparse_csr()
    base = (dense.double() @ s_d.double())
    res = {"device": torch.cuda.get_device_name(0), "repeats": a.repeats, "N": a.N, "P": a.P, "members": nnz,
           "sizes": "log-uniform in [10, 500]", "torch_chunk": a.chunk, "clocks_before": clocks(),
           "library_sha256": hashlib.sha256(open(_lib.lib_path(), "rb").read()).hexdigest(), "rows": []}
    for R in (int(v) for v in a.R.split(",")):
        whole = lambda: pa.pathway_permutation_test(scores, pw, n_perm=R, seed=1, device=dev)       # noqa: E731
        call = lambda: engine.pathway_permutations(s_d, ptr_d, idx_d, 1, 0, R)                    # noqa: E731
        t_whole, t_call = timed(whole, a.repeats), timed(call, a.repeats)
        stage_ms = []
        os.environ["PHX_DIAG"] = "1"
        try:
            for stage in (1, 2, 3):
                os.environ["PHX_PATHWAYS_STAGES"] = str(stage)
                stage_ms.append(med(timed(call, a.repeats)))
        finally:
            del os.environ["PHX_DIAG"], os.environ["PHX_PATHWAYS_STAGES"]
        stage_ms.append(med(t_call))
        shares = dict(zip(STAGES, np.diff([0.0] + stage_ms).tolist()))
        Rt = min(R, a.torch_perms)
        t_dense = med(timed(lambda: torch_form(s_d, dense, base, Rt, a.chunk, False), a.repeats, warmup=1))
        t_sparse = med(timed(lambda: torch_form(s_d, csr, base, Rt, a.chunk, True), a.repeats, warmup=1))
        row = {"R": R, "pathway_permutation_test_ms": med(t_whole), "kernel_call_ms": med(t_call), "kernel_call_all_ms": t_call,
               "ended_after_stage_ms": dict(zip(STAGES, stage_ms)), "stage_share_ms": shares,
               "lds_gather_GBps": nnz * R * 4 / (shares["walk"] * 1e-3) / 1e9 if shares["walk"] > 0 else None,
               "torch_permutations_timed": Rt, "torch_dense_ms_scaled_to_R": t_dense * R / Rt,
               "torch_sparse_ms_scaled_to_R": t_sparse * R / Rt,
               "kernel_over_better_torch": med(t_call) / (min(t_dense, t_sparse) * R / Rt),
               "workspace_bytes": int(_lib.load().phx_pathway_permutations_workspace_bytes(a.N, a.P, nnz, R))}
        res["rows"].append(row)
        print("R=%d: pathway_permutation_test %.2f ms, kernel call %.2f ms (keys %.2f, sort %.2f, image %.2f, walk %.2f; LDS gather "
              "%.0f GB/s); torch dense %.1f ms, sparse %.1f ms (timed over %d permutations, scaled)"
              % (R, med(t_whole), med(t_call), shares["keys"], shares["sort"], shares["image"], shares["walk"],
                 row["lds_gather_GBps"] or 0.0, row["torch_dense_ms_scaled_to_R"], row["torch_sparse_ms_scaled_to_R"], Rt), flush=True)
    res["clocks_after"] = clocks()
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
