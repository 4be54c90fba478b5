#!/usr/bin/env python3
"""Per-gene neighbour lists, `effects_neighbors` against the composition it replaces (run on the MI355X):
    python tools/bench_neighbors.py [--shapes 11165x40,14691x200] [--B 60] [--k 20] [--repeats 10] [--out profiles/effects_neighbors.json]
Per shape (N, H), for the effects matrix and for the mean |Jacobian| over B states, for both axes, with and without `orient`:
  - `effects_neighbors(k)` as a whole (the candidate-free call: one selection launch, one merge launch, two dtype casts);
  - the composition available without it: `effects_matrix` / `jacobian_matrix` in row chunks, abs(), torch.topk -- along the
    rows of a chunk for of="regulator", a running merge of the chunks' column-wise topk for of="target" -- and the degree and
    weighted degree by sums; `orient` needs the transposed comparison and therefore the whole matrix at once;
  - phx_effects_matrix of the same mode in the same run (the selection does that kernel's MFMA work without its store,
    twice with `orient`);
  - the peak device memory of both beyond what is allocated before the call, and the size of the workspace the engine keeps
    cached between calls (the segments' lists), which that figure does not see.
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


def composition(p, mode, y, ph, of, orient, k):
    """what a caller of `effects_matrix` / `jacobian_matrix` does to get every line's k strongest entries, count and sum"""
    N, dev = p.N, p.device
    if orient:
        M = engine.effects_matrix(p, mode, y=y, ph=ph)
        mag = M.abs()
        mag = torch.where(mag > mag.t(), mag, torch.zeros((), device=dev))
        dim = 0 if of == "target" else 1
        top = torch.topk(mag, k, dim=dim)
        return top.indices, top.values, (mag > 0).sum(dim), mag.sum(dim)
    count = torch.zeros(N, dtype=torch.int64, device=dev)
    strength = torch.zeros(N, dtype=torch.float32, device=dev)
    best_v = best_i = None
    pieces = []
    for r0 in range(0, N, CHUNK):
        r1 = min(N, r0 + CHUNK)
        mag = engine.effects_matrix(p, mode, y=y, ph=ph, rows=(r0, r1)).abs()
        rows = torch.arange(r0, r1, device=dev)
        mag[rows - r0, rows] = 0                                   # the diagonal
        if of == "regulator":
            top = torch.topk(mag, k, dim=1)
            pieces.append((top.indices, top.values))
            count[r0:r1] = (mag > 0).sum(1)
            strength[r0:r1] = mag.sum(1)
        else:
            top = torch.topk(mag, min(k, r1 - r0), dim=0)
            v, i = top.values, top.indices + r0
            if best_v is not None:
                v, i = torch.cat((best_v, v)), torch.cat((best_i, i))
                keep = torch.topk(v, k, dim=0)
                v, i = keep.values, torch.gather(i, 0, keep.indices)
            best_v, best_i = v, i
            count += (mag > 0).sum(0)
            strength += mag.sum(0)
    if of == "regulator":
        return torch.cat([x[0] for x in pieces]), torch.cat([x[1] for x in pieces]), count, strength
    return best_i, best_v, count, strength


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="11165x40,14691x200")
    ap.add_argument("--B", type=int, default=60)
    ap.add_argument("--k", type=int, default=20)
    ap.add_argument("--repeats", type=int, default=10)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "effects_neighbors.json"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("bench_neighbors.py measures on the GPU; none is visible")
    dev = torch.device("cuda:0")
    med = lambda v: float(np.median(v))                            # noqa: E731
    res = {"device": torch.cuda.get_device_name(0), "repeats": a.repeats, "B": a.B, "k": a.k, "chunk_rows": CHUNK,
           "library_sha256": hashlib.sha256(open(_lib.lib_path(), "rb").read()).hexdigest(), "rows": []}
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
            for of in ("target", "regulator"):
                for orient in (False, True):
                    kernel = lambda: engine.effects_neighbors(p, mode, a.k, of=of, y=y, ph=ph, orient=orient)   # noqa: E731
                    comp = lambda: composition(p, mode, y, ph, of, orient, a.k)                                 # noqa: E731
                    got, ref = kernel(), comp()
                    ref_mag = ref[1].t() if of == "target" else ref[1]
                    same = bool(torch.equal(got[1].abs(), ref_mag)) and bool(torch.equal(got[2], ref[2]))
                    del got, ref, ref_mag
                    t_kernel, t_comp = timed(kernel, a.repeats), timed(comp, a.repeats)
                    m_kernel, m_comp = peak_growth(kernel), peak_growth(comp)
                    row = {"N": N, "H": H, "mode": mode, "B": B, "of": of, "orient": orient, "k": a.k, "matrix_bytes": 4 * N * N,
                           "effects_matrix_ms": t_matrix, "effects_neighbors_ms": med(t_kernel), "composition_ms": med(t_comp),
                           "neighbors_over_matrix": med(t_kernel) / t_matrix, "neighbors_over_composition": med(t_kernel) / med(t_comp),
                           "effects_neighbors_peak_bytes": m_kernel, "composition_peak_bytes": m_comp,
                           "cached_workspace_bytes": int(_lib.load().phx_effects_neighbors_workspace_bytes(
                               N, H, B, _lib.EFFECTS_MODES[mode], _lib.NEIGHBORS_AXES[of], a.k)),
                           "same_magnitudes_and_counts_as_composition": same, "effects_neighbors_all_ms": t_kernel}
                    res["rows"].append(row)
                    print("N=%d H=%d %s of=%s orient=%d: matrix kernel %.3f ms; effects_neighbors %.3f ms (%.2fx) / %.2f MB, "
                          "composition %.3f ms / %.1f MB; same magnitudes and counts: %s"
                          % (N, H, mode, of, orient, t_matrix, med(t_kernel), med(t_kernel) / t_matrix, m_kernel / 1e6, med(t_comp),
                             m_comp / 1e6, same), flush=True)
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
