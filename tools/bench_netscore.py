#!/usr/bin/env python3
"""Network scoring, `network_score` against the composition it replaces (run on the MI355X):
    python tools/bench_netscore.py [--shapes 11165x40,14691x200] [--B 60] [--labels 100000,1000000] [--out profiles/netscore.json]
Per shape (N, H), for the effects matrix and for the mean |Jacobian| over B states, per label-set size (seeded random
off-diagonal pairs):
  - the GATHER pass and the RANK pass of phx_netscore.hip alone, against phx_effects_matrix of the same mode in the same
    run (a pass does that kernel's MFMA work without its store);
  - `network_score` as a whole (label sort, both passes, the host read of the non-finite counter, the cumulative sums);
  - the composition available without it, on the same device: the dense matrix, torch.sort of the N^2 magnitudes, cumulative
    sums of the sorted labels, the same AUROC from them;
  - the peak device memory of both beyond what is allocated before the call.
Warm-up 1, best of 3, HIP events.  Reads nothing outside the tree; writes one JSON file."""
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
import phoenix_amd as pa                                           # noqa: E402
from phoenix_amd import _lib, engine                               # noqa: E402
from phoenix_amd.odenet import params_of                           # noqa: E402
from tools.bench_edges import peak_growth                          # noqa: E402
from tools.bench_effects import timed                              # noqa: E402


def composition(p, mode, y, ph, reg, tgt):
    """AUROC of the off-diagonal magnitudes by a full sort: what a caller of `effects_matrix` / `jacobian_matrix` can do"""
    N = p.N
    M = engine.effects_matrix(p, mode, y=y, ph=ph)
    label = torch.zeros((N, N), dtype=torch.bool, device=M.device)
    label[reg, tgt] = True
    off = ~torch.eye(N, dtype=torch.bool, device=M.device)
    mag, lab = M.abs()[off], label[off]
    del M, label, off
    mag, order = torch.sort(mag)
    lab = lab[order]
    del order
    # mid-ranks of the tie groups, then the Mann-Whitney statistic of the positives
    _, inv, cnt = torch.unique_consecutive(mag, return_inverse=True, return_counts=True)
    hi = torch.cumsum(cnt, 0)
    mid = (hi - cnt).to(torch.float64) + (cnt.to(torch.float64) + 1) / 2
    P = int(lab.sum())
    Nn = lab.numel() - P
    U = float(mid[inv][lab].sum()) - P * (P + 1) / 2
    return U / (P * Nn)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="11165x40,14691x200")
    ap.add_argument("--B", type=int, default=60)
    ap.add_argument("--labels", default="100000,1000000")
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "netscore.json"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("bench_netscore.py measures on the GPU; none is visible")
    dev = torch.device("cuda:0")
    lib = _lib.load()
    best = lambda v: float(np.min(v))                              # noqa: E731
    res = {"device": torch.cuda.get_device_name(0), "repeats": a.repeats, "warmup": 1, "statistic": "best", "B": a.B,
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
        ws = torch.zeros(32, dtype=torch.int32, device=dev)
        for mode in ("effects", "mean_abs"):
            y, ph, B = (None, None, 1) if mode == "effects" else (yB, phB, a.B)
            out = torch.empty((N, N), device=dev)
            t_matrix = best(timed(lambda: engine.effects_matrix(p, mode, y=y, ph=ph, out=out), a.repeats, warmup=1))
            del out
            for E in (int(v) for v in a.labels.split(",")):
                gen = torch.Generator(device=dev).manual_seed(E)
                key = torch.unique(torch.randint(0, N * N, (E,), device=dev, generator=gen))
                key = key[key % (N + 1) != 0]
                reg, tgt = key // N, key % N
                for orient in (False, True):
                    flags = _lib.EDGES_ORIENT if orient else 0
                    got = engine.network_score(p, mode, reg, tgt, y=y, ph=ph, orient=orient)
                    auroc_comp = None if orient else composition(p, mode, y, ph, reg, tgt)
                    # the two passes alone, on the inputs network_score gives them
                    vals = engine.effects_gather(p, mode, reg, tgt, y=y, ph=ph, orient=orient)
                    u = torch.unique(vals.view(torch.int32) & 0x7FFFFFFF)
                    counts = torch.empty(2 * u.numel() + 1, dtype=torch.int32, device=dev)
                    t_gather = best(timed(lambda: engine.effects_gather(p, mode, reg, tgt, y=y, ph=ph, orient=orient),
                                          a.repeats, warmup=1))

                    def rank():
                        rc = lib.phx_effects_rank_counts(C.byref(p.c), _lib.EFFECTS_MODES[mode], engine._p(y), engine._p(ph), B,
                                                         flags, engine._p(u), u.numel(), engine._p(counts), engine._p(ws),
                                                         ws.numel() * 4, engine._stream_ptr())
                        assert rc == 0, rc
                    t_rank = best(timed(rank, a.repeats, warmup=1))
                    score = lambda: engine.network_score(p, mode, reg, tgt, y=y, ph=ph, orient=orient)   # noqa: E731
                    t_all = timed(score, a.repeats, warmup=1)
                    m_score = peak_growth(score)
                    row = {"N": N, "H": H, "mode": mode, "B": B, "orient": orient, "labels": int(key.numel()),
                           "distinct_positive_magnitudes": int(u.numel()), "matrix_bytes": 4 * N * N,
                           "effects_matrix_ms": t_matrix, "gather_with_label_sort_ms": t_gather, "rank_pass_ms": t_rank,
                           "rank_over_matrix": t_rank / t_matrix, "network_score_ms": best(t_all),
                           "network_score_peak_bytes": m_score, "auroc": got[0], "average_precision": got[1],
                           "network_score_all_ms": t_all}
                    if not orient:
                        t_comp = timed(lambda: composition(p, mode, y, ph, reg, tgt), a.repeats, warmup=1)
                        row.update({"composition_ms": best(t_comp), "composition_peak_bytes":
                                    peak_growth(lambda: composition(p, mode, y, ph, reg, tgt)), "composition_auroc": auroc_comp,
                                    "score_over_composition": best(t_all) / best(t_comp)})
                    res["rows"].append(row)
                    print(json.dumps({k: v for k, v in row.items() if k != "network_score_all_ms"}), flush=True)
                    del vals, u, counts
        del net, p
        engine.forget_params()
        torch.cuda.empty_cache()
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
