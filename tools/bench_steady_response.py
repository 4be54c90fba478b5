#!/usr/bin/env python3
"""`steady_state_response` against what a caller had before it (run on the MI355X):
    python tools/bench_steady_response.py [--shapes 11165x40x60,14691x200x24] [--knockouts 64] [--repeats 5]
                                          [--out profiles/steady_response.json]
Per shape (N, H, states), on the model and the states of tools/bench_steady.py, relaxed by `steady_states`; all N
regulators, input="level", reduce="mean_abs":
  - the whole call and each of its stages (phx_reduced_jacobian, phx_steady_inverse, phx_steady_response_factors and
    phx_steady_response per block of regulators and summed over the blocks), and what share of the 157.3 TFLOP/s fp32 MFMA
    peak the hot kernel's 4 H K N B flops come to;
  - the same matrix with torch on the same device: per state S by a matmul, Z C by `torch.linalg.solve` in float64, one
    `matmul` to an N x N temporary, `abs_` and an addition;
  - `knockout_steady_states` of `knockouts` genes: the finite perturbations the matrix linearises, one Newton solve each,
    with the passes its slowest row needs.
Warm-up, HIP events, medians of the repeats; a line is printed after every figure and the JSON file is rewritten after every
shape, so a run that is cut short keeps what it had.  A figure that could not be taken is the string "not measured" with the
reason beside it.  Reads nothing outside the tree; writes one JSON file."""
import argparse
import hashlib
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
import phoenix_amd as pa                                           # noqa: E402
from phoenix_amd import _lib, engine                               # noqa: E402
from phoenix_amd.odenet import params_of                           # noqa: E402
from bench_steady import PEAK, TOL, model, timed                   # noqa: E402


def say(*what):
    print(*what, flush=True)


def torch_response(net, y, free):
    """the baseline -> response [N, N] (level, mean_abs), every row used"""
    ws, bs, wp, bp, wa, g = (x.detach() for x in params_of(net))
    H, N = ws.shape
    B = y.shape[0]
    m = free.float()
    s = y - 0.5
    d = 1 + s.abs()
    a = s / d
    da = 1 / (d * d)
    dl = da / (1 + a)
    v = torch.exp(torch.log1p(a) @ wp.t() + bp)
    eye = torch.eye(2 * H, device=y.device, dtype=torch.float64)
    acc = torch.zeros((N, N), device=y.device)
    diag = torch.arange(N, device=y.device)
    for b in range(B):
        C = torch.cat([ws * da[b], v[b].unsqueeze(1) * wp * dl[b]], dim=0)               # [2H, N]
        S = (C * m[b]) @ wa
        X = torch.linalg.solve(eye - S.double(), C.double()).float()                   # Z C
        dd = 1 + m[b] * (wa * X.t()).sum(dim=1)
        T = (X / dd).t() @ wa.t()                                                     # [regulator, target]
        T.mul_(m[b]).abs_()
        acc += T
    acc /= B
    acc[diag, diag] = 1.0
    return acc


def measure(shape, K, repeats, dev):
    N, H, states = (int(v) for v in shape.split("x"))
    med = lambda v: float(np.median(v))                            # noqa: E731
    row = {"N": N, "H": H, "states": states, "regulators": N}
    say("case", row)

    def put(**kw):
        row.update(kw)
        say("  " + json.dumps(kw))
    net = model(N, H, dev)
    y0 = torch.rand((states, N), device=dev, generator=torch.Generator(dev).manual_seed(N))
    st = pa.steady_states(net, y0, tol=TOL)
    put(converged_rows=int((st.status == 0).sum()), steps=int(st.iterations.max()))
    with torch.no_grad():
        P = engine.params_cached(*params_of(net))
        free = (P.g > 0).reshape(1, -1).repeat(states, 1)
        m = free.float()
        call = lambda: pa.steady_state_response(net, st.y, status=st.status)           # noqa: E731
        out = call()
        put(rows_used=int((out.info == 0).sum()), steady_state_response_ms=med(timed(call, repeats, warmup=1)))
        S, _, hid = engine.reduced_jacobian(P, st.y, m)
        Z, info = engine.steady_inverse(S)
        block = max(1, (256 << 20) // (states * 2 * H * 4))
        block = block // 64 * 64 if block >= 64 else block
        genes = torch.arange(N, dtype=torch.int32, device=dev)
        blocks = [genes[k0:k0 + block] for k0 in range(0, N, block)]
        put(reduced_jacobian_ms=med(timed(lambda: engine.reduced_jacobian(P, st.y, m), repeats)),
            inverse_ms=med(timed(lambda: engine.steady_inverse(S), repeats)), regulator_blocks=len(blocks), block=min(block, N))
        f_ms = h_ms = 0.0
        res = torch.empty((N, N), device=dev)
        for k0, gb in zip(range(0, N, block), blocks):
            X, use = engine.steady_response_factors(P, st.y, m, hid, Z, info, gb, "level")
            f_ms += med(timed(lambda: engine.steady_response_factors(P, st.y, m, hid, Z, info, gb, "level"), repeats, warmup=1))
            h_ms += med(timed(lambda: engine.steady_response(P, m, X, use, gb, "level", True, res[k0:k0 + len(gb)]), repeats, warmup=1))
            del X, use
        flops = 4.0 * H * N * N * states
        put(factors_ms=f_ms, response_kernel_ms=h_ms, response_kernel_flops=flops,
            response_kernel_fraction_of_peak=flops / (h_ms * 1e-3) / PEAK, same_bits_as_the_call=bool(torch.equal(res, out.response)))
        del res
        try:
            base = torch_response(net, st.y, free)
            put(torch_distance=float((base - out.response).abs().max()), largest_entry_off_diagonal=float(
                (out.response - torch.eye(N, device=dev)).abs().max()))
            del base
            put(torch_ms=med(timed(lambda: torch_response(net, st.y, free), max(1, repeats // 2), warmup=1)))
        except Exception as e:                                      # noqa: BLE001
            put(torch_ms="not measured", torch_reason=repr(e)[:300])
        try:
            # (all max_iter passes are issued whether a row still moves or not: the passes the slowest row needs are found first)
            full = pa.knockout_steady_states(net, y0, list(range(K)), tol=TOL, max_iter=16)
            steps = int(max(full.base.iterations.max(), full.knockouts.iterations.max()))
            ko = lambda: pa.knockout_steady_states(net, y0, list(range(K)), tol=TOL, max_iter=steps)    # noqa: E731
            put(knockouts=K, knockout_steps=steps, knockout_rows_converged=int((full.knockouts.status == 0).sum()),
                knockout_steady_states_ms=med(timed(ko, max(1, repeats // 2), warmup=1)))
        except Exception as e:                                      # noqa: BLE001
            put(knockout_steady_states_ms="not measured", knockout_reason=repr(e)[:300])
    return row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="11165x40x60,14691x200x24")
    ap.add_argument("--knockouts", type=int, default=64)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "steady_response.json"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("bench_steady_response.py measures on the GPU; none is visible")
    dev = torch.device("cuda:0")
    res = {"device": torch.cuda.get_device_name(0), "repeats": a.repeats, "tol": TOL, "fp32_mfma_peak_flops": PEAK,
           "input": "level", "reduce": "mean_abs",
           "library_sha256": hashlib.sha256(open(_lib.lib_path(), "rb").read()).hexdigest(), "rows": []}
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    for shape in a.shapes.split(","):
        res["rows"].append(measure(shape, a.knockouts, a.repeats, dev))
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)
    say("wrote", a.out)


if __name__ == "__main__":
    main()
