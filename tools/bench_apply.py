#!/usr/bin/env python3
"""Matrix-free products with the inferred network, `effects_apply` against the composition it replaces (run on the MI355X):
    python tools/bench_apply.py [--shapes 11165x40,14691x200] [--B 60] [--R 1,8,32] [--repeats 10] [--out profiles/effects_apply.json]
Per shape (N, H), for the effects matrix and for the mean |Jacobian| over B states, for R columns, with and without `orient`
(of="target", weight="abs": the product a downstream walk takes):
  - one prepared `effects_apply` (engine.ApplyOperator.apply: one product launch, one launch that adds the segments);
  - the composition available without it: `effects_matrix` / `jacobian_matrix` in 2048-row chunks, abs(), the diagonal off,
    one `matmul` per chunk; `orient` needs the transposed comparison and therefore the whole matrix at once;
  - phx_effects_matrix of the same mode in the same run (the product does that kernel's MFMA work without its store, twice
    with `orient`);
  - the peak device memory of both beyond what is allocated before the call, and the size of the cached workspace;
  - a 20-step `network_propagation` from three seed genes (22 products: 20 steps and the strengths).
Warm-up, HIP events, median of the repeats.  Reads nothing outside the tree; writes one JSON file."""
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
from phoenix_amd.odenet import params_of                           # noqa: E402
from tools.bench_edges import peak_growth                          # noqa: E402
from tools.bench_effects import timed                              # noqa: E402

CHUNK = 2048       # regulator rows of a piece of the matrix in the composition


def composition(p, mode, y, ph, orient, V):
    """what a caller of `effects_matrix` / `jacobian_matrix` does for |M|^T V over the eligible entries"""
    N, dev = p.N, p.device
    if orient:
        mag = engine.effects_matrix(p, mode, y=y, ph=ph).abs()
        mag = torch.where(mag > mag.t(), mag, torch.zeros((), device=dev))
        return mag.t() @ V
    out = torch.zeros_like(V)
    for r0 in range(0, N, CHUNK):
        r1 = min(N, r0 + CHUNK)
        mag = engine.effects_matrix(p, mode, y=y, ph=ph, rows=(r0, r1)).abs()
        rows = torch.arange(r0, r1, device=dev)
        mag[rows - r0, rows] = 0                                   # the diagonal
        out.addmm_(mag.t(), V[r0:r1])
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="11165x40,14691x200")
    ap.add_argument("--B", type=int, default=60)
    ap.add_argument("--R", default="1,8,32")
    ap.add_argument("--repeats", type=int, default=10)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "effects_apply.json"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("bench_apply.py measures on the GPU; none is visible")
    dev = torch.device("cuda:0")
    med = lambda v: float(np.median(v))                            # noqa: E731
    res = {"device": torch.cuda.get_device_name(0), "repeats": a.repeats, "B": a.B, "chunk_rows": CHUNK,
           "library_sha256": hashlib.sha256(open(_lib.lib_path(), "rb").read()).hexdigest(), "rows": [], "propagation": []}
    for shape in a.shapes.split(","):
        N, H = (int(v) for v in shape.split("x"))
        torch.manual_seed(0)
        net = pa.ODENet(dev, N, neurons=H)
        with torch.no_grad():                                      # dense, trained-like weights
            for lin in (net.net_sums.linear_out, net.net_prods.linear_out, net.net_alpha_combine.linear_out):
                lin.weight.normal_(0.0, 0.6 / np.sqrt(N))
            net.gene_multipliers.sub_(0.2)
        p = engine.params_cached(*params_of(net))
        yB = torch.rand((a.B, N), device=dev) * 1.4 - 0.2
        s = yB - 0.5
        phB = torch.exp(torch.addmm(p.bp, torch.log1p(s / (1 + s.abs())), p.Wp.t()))
        for mode in ("effects", "mean_abs"):
            y, ph, B = (None, None, 1) if mode == "effects" else (yB, phB, a.B)
            out = torch.empty((N, N), device=dev)
            t_matrix = med(timed(lambda: engine.effects_matrix(p, mode, y=y, ph=ph, out=out), a.repeats))
            del out
            for orient in (False, True):
                op = engine.ApplyOperator(p, mode, y=y, ph=ph, orient=orient)
                for R in (int(r) for r in a.R.split(",")):
                    V = torch.rand((N, R), device=dev)
                    kernel = lambda: op.apply(V, "target", "abs")                            # noqa: E731
                    comp = lambda: composition(p, mode, y, ph, orient, V)                    # noqa: E731
                    got, ref = kernel(), comp()
                    diff = float(((got - ref).abs().max() / ref.abs().max()).item())
                    del got, ref
                    t_kernel, t_comp = timed(kernel, a.repeats), timed(comp, a.repeats)
                    m_kernel, m_comp = peak_growth(kernel), peak_growth(comp)
                    row = {"N": N, "H": H, "mode": mode, "B": B, "orient": orient, "R": R, "matrix_bytes": 4 * N * N,
                           "effects_matrix_ms": t_matrix, "effects_apply_ms": med(t_kernel), "composition_ms": med(t_comp),
                           "apply_over_matrix": med(t_kernel) / t_matrix, "apply_over_composition": med(t_kernel) / med(t_comp),
                           "effects_apply_peak_bytes": m_kernel, "composition_peak_bytes": m_comp,
                           "cached_workspace_bytes": int(_lib.load().phx_effects_apply_workspace_bytes(
                               N, H, B, _lib.EFFECTS_MODES[mode], _lib.NEIGHBORS_AXES["target"], R)),
                           "max_norm_difference_from_composition": diff, "effects_apply_all_ms": t_kernel}
                    res["rows"].append(row)
                    print("N=%d H=%d %s orient=%d R=%d: matrix kernel %.3f ms; effects_apply %.3f ms (%.2fx) / %.2f MB, "
                          "composition %.3f ms / %.1f MB; max-norm difference %.2e"
                          % (N, H, mode, orient, R, t_matrix, med(t_kernel), med(t_kernel) / t_matrix, m_kernel / 1e6, med(t_comp),
                             m_comp / 1e6, diff), flush=True)
                kw = dict(orient=orient) if mode == "effects" else dict(orient=orient, y=yB, reduce=mode)
                walk = lambda: pa.network_propagation(net, [1, 2, 3], iterations=20, **kw)   # noqa: E731
                t_walk = timed(walk, a.repeats)
                res["propagation"].append({"N": N, "H": H, "mode": mode, "B": B, "orient": orient, "iterations": 20,
                                           "network_propagation_ms": med(t_walk), "over_matrix": med(t_walk) / t_matrix,
                                           "peak_bytes": peak_growth(walk), "network_propagation_all_ms": t_walk})
                print("N=%d H=%d %s orient=%d: 20-step network_propagation %.3f ms (%.2fx the matrix kernel)"
                      % (N, H, mode, orient, med(t_walk), med(t_walk) / t_matrix), flush=True)
        del net, p
        engine.forget_params()
        engine.forget_workspaces()
        torch.cuda.empty_cache()
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
