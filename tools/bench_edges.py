#!/usr/bin/env python3
"""Edge extraction, `effects_edges` against the composition it replaces (run on the MI355X):
    python tools/bench_edges.py [--shapes 11165x40,14691x200] [--B 60] [--top 100000] [--repeats 10] [--out profiles/effects_edges.json]
Per shape (N, H), for the effects matrix and for the mean |Jacobian| over B states, with and without `orient`:
  - the COUNT pass and the EMIT pass of phx_effects_edges alone, each against phx_effects_matrix of the same mode in the
    same run (a pass does that kernel's MFMA work without its store);
  - `effects_edges(top=K)` as a whole (passes, host reads of the histogram and the count, the sort);
  - the composition available without it: the dense matrix, abs(), the transposed comparison for `orient`, topk;
  - the peak device memory of both beyond what is allocated before the call.
Warm-up, HIP events, median of the repeats.  Reads nothing outside the tree; writes one JSON file."""
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
from tools.bench_effects import timed                              # noqa: E402


def peak_growth(fn):
    torch.cuda.synchronize()
    torch.cuda.empty_cache()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    out = fn()
    torch.cuda.synchronize()
    grown = torch.cuda.max_memory_allocated() - base
    del out
    return int(grown)


def composition(p, mode, y, ph, orient, K):
    """what a caller of `effects_matrix` / `jacobian_matrix` does to get the K strongest edges"""
    M = engine.effects_matrix(p, mode, y=y, ph=ph)
    mag = M.abs()
    mag.fill_diagonal_(0)
    if orient:
        mag = torch.where(mag > mag.t(), mag, torch.zeros((), device=mag.device))
    top = torch.topk(mag.reshape(-1), K)
    return top.indices // p.N, top.indices % p.N, M.reshape(-1)[top.indices]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="11165x40,14691x200")
    ap.add_argument("--B", type=int, default=60)
    ap.add_argument("--top", type=int, default=100000)
    ap.add_argument("--repeats", type=int, default=10)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "effects_edges.json"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("bench_edges.py measures on the GPU; none is visible")
    dev = torch.device("cuda:0")
    lib = _lib.load()
    med = lambda v: float(np.median(v))                            # noqa: E731
    res = {"device": torch.cuda.get_device_name(0), "repeats": a.repeats, "B": a.B, "top": a.top,
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
        ws = torch.zeros(_lib.EDGES_BINS + 16, dtype=torch.int32, device=dev)
        keys = torch.empty(4 * a.top, dtype=torch.int64, device=dev)
        vals = torch.empty(4 * a.top, dtype=torch.float32, device=dev)
        for mode in ("effects", "mean_abs"):
            y, ph, B = (None, None, 1) if mode == "effects" else (yB, phB, a.B)
            out = torch.empty((N, N), device=dev)
            t_matrix = med(timed(lambda: engine.effects_matrix(p, mode, y=y, ph=ph, out=out), a.repeats))
            del out
            for orient in (False, True):
                got = engine.effects_edges(p, mode, y=y, ph=ph, top=a.top, orient=orient)
                ref = composition(p, mode, y, ph, orient, a.top)
                same = bool(torch.equal(got[2].abs(), ref[2].abs()))     # (topk orders equal magnitudes as it likes)
                tau = float(got[2][-1].abs())
                flags = _lib.EDGES_ORIENT if orient else 0

                def one_pass(pass_):
                    rc = lib.phx_effects_edges(C.byref(p.c), _lib.EFFECTS_MODES[mode], engine._p(y), engine._p(ph), B, flags,
                                               pass_, 0, 0, tau, engine._p(keys), engine._p(vals), keys.numel(), engine._p(ws),
                                               ws.numel() * 4, engine._stream_ptr())
                    assert rc == 0, rc
                t_count = med(timed(lambda: one_pass(_lib.EDGES_COUNT), a.repeats))
                t_emit = med(timed(lambda: one_pass(_lib.EDGES_EMIT), a.repeats))
                emitted = int(ws[_lib.EDGES_BINS].item())
                t_all = timed(lambda: engine.effects_edges(p, mode, y=y, ph=ph, top=a.top, orient=orient), a.repeats)
                t_comp = timed(lambda: composition(p, mode, y, ph, orient, a.top), a.repeats)
                m_edges = peak_growth(lambda: engine.effects_edges(p, mode, y=y, ph=ph, top=a.top, orient=orient))
                m_comp = peak_growth(lambda: composition(p, mode, y, ph, orient, a.top))
                row = {"N": N, "H": H, "mode": mode, "B": B, "orient": orient, "matrix_bytes": 4 * N * N,
                       "effects_matrix_ms": t_matrix, "count_pass_ms": t_count, "emit_pass_ms": t_emit,
                       "count_over_matrix": t_count / t_matrix, "emit_over_matrix": t_emit / t_matrix,
                       "emitted_at_the_weakest_edge": emitted, "effects_edges_ms": med(t_all), "composition_ms": med(t_comp),
                       "edges_over_composition": med(t_all) / med(t_comp), "effects_edges_peak_bytes": m_edges,
                       "composition_peak_bytes": m_comp, "same_magnitudes_as_composition": same, "effects_edges_all_ms": t_all}
                res["rows"].append(row)
                print("N=%d H=%d %s orient=%d: matrix kernel %.3f ms, count %.3f (%.2fx), emit %.3f (%.2fx); effects_edges %.3f ms "
                      "/ %.2f MB, composition %.3f ms / %.1f MB; same magnitudes: %s"
                      % (N, H, mode, orient, t_matrix, t_count, t_count / t_matrix, t_emit, t_emit / t_matrix, med(t_all),
                         m_edges / 1e6, med(t_comp), m_comp / 1e6, same), flush=True)
        del net, p, keys, vals
        engine.forget_params()
        torch.cuda.empty_cache()
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
