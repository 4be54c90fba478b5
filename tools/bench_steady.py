#!/usr/bin/env python3
"""Steady states by implicit relaxation, `steady_states` against what a caller had before it (run on the MI355X):
    python tools/bench_steady.py [--shapes 11165x40x60,14691x200x24] [--repeats 5] [--out profiles/steady_states.json]
Per shape (N, H, B), on a model of the tests' recipe (tests/test_steady_cpu.py: make_model) from y0 ~ U[0, 1):
  - phx_reduced_jacobian alone (the S kernel and the launch that adds its segments), and what fraction of the 157.3 TFLOP/s
    fp32 MFMA peak its 8 H^2 N B flops come to;
  - the whole solve: `steady_states` with max_iter = the steps its slowest row needs (a first run finds them; every pass
    costs the same whether a row is still moving or frozen), hence the time per iteration;
  - the same iteration with S, w formed by `torch.einsum` and the 2H x 2H systems solved by `torch.linalg.solve`;
  - an `odeint(..., dopri5)` call long enough to reach the same residual: T doubles from 15 until the largest residual over the
    rows is at or below that of `steady_states` (or tol), at most to 240.
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

PEAK = 157.3e12
TOL = 1e-5


def timed(fn, repeats, warmup=2):
    for _ in range(warmup):
        fn()
    ms = []
    for _ in range(repeats):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        ms.append(a.elapsed_time(b))
    return ms


def model(N, H, dev):
    """the tests' recipe: Ws, Wp ~ N(0, (c1 / sqrt N)^2), Wa ~ N(0, (c2 / sqrt 2H)^2), small biases, g ~ U(0.2, 1.2) with N // 16
    entries negated"""
    c1, c2 = (1.5, 0.6) if H <= 56 else (1.0, 0.45)
    gen = torch.Generator().manual_seed(N + H)
    net = pa.ODENet(dev, N, neurons=H)
    with torch.no_grad():
        net.net_sums.linear_out.weight.copy_(torch.randn((H, N), generator=gen) * c1 / N ** 0.5)
        net.net_prods.linear_out.weight.copy_(torch.randn((H, N), generator=gen) * c1 / N ** 0.5)
        net.net_alpha_combine.linear_out.weight.copy_(torch.randn((N, 2 * H), generator=gen) * c2 / (2 * H) ** 0.5)
        net.net_sums.linear_out.bias.copy_(torch.rand(H, generator=gen) * 0.2 - 0.1)
        net.net_prods.linear_out.bias.copy_(torch.rand(H, generator=gen) * 0.2 - 0.1)
        g = torch.rand(N, generator=gen) + 0.2
        g[torch.randperm(N, generator=gen)[:max(1, N // 16)]] *= -1
        net.gene_multipliers.copy_(g.reshape(1, N))
    return net


def einsum_iteration(net, y0, free, steps):
    """the iteration of phoenix_amd.steady with torch alone: C formed per state, S and w by einsum, a batched dense solve"""
    ws, bs, wp, bp, wa, g = (x.detach() for x in params_of(net))
    gf = torch.where(free, torch.relu(g).reshape(1, -1), torch.zeros((), device=y0.device))

    def state(y):
        s = y - 0.5
        d = 1 + s.abs()
        a = s / d
        v = torch.exp(torch.log1p(a) @ wp.t() + bp)
        da = 1 / (d * d)
        r = torch.cat([a @ ws.t() + bs, v], dim=1) @ wa.t() - y
        return r, torch.where(free, r.abs(), 0.0).amax(dim=1), da, da / (1 + a), v

    y, tau = y0.clone(), torch.ones(y0.shape[0], device=y0.device)
    r, rho, da, dl, v = state(y)
    eye = torch.eye(2 * ws.shape[0], device=y0.device, dtype=torch.float64)
    for _ in range(steps):
        tg = tau.unsqueeze(1) * gf
        m = tg / (1 + tg)
        S = torch.cat([torch.einsum("jn,bn,nc->bjc", ws, da * m, wa), v.unsqueeze(2) * torch.einsum("jn,bn,nc->bjc", wp, dl * m, wa)],
                      dim=1)
        mr = m * r
        w = torch.cat([(da * mr) @ ws.t(), v * ((dl * mr) @ wp.t())], dim=1)
        x = torch.linalg.solve(eye - S.double(), w.double()).float()
        yc = torch.where(free, y + m * (r + x @ wa.t()), y)
        rc, rhoc, dac, dlc, vc = state(yc)
        ok = torch.isfinite(rhoc) & (rhoc <= 2 * rho) & (rho > TOL)
        tau = torch.where(ok, tau * torch.clamp(rho / rhoc, 2.0, 10.0), torch.where(rho > TOL, tau / 4, tau))
        o = ok.unsqueeze(1)
        y, r, da, dl, v = (torch.where(o, n, c) for n, c in ((yc, y), (rc, r), (dac, da), (dlc, dl), (vc, v)))
        rho = torch.where(ok, rhoc, rho)
    return y, rho


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="11165x40x60,14691x200x24")
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "steady_states.json"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("bench_steady.py measures on the GPU; none is visible")
    dev = torch.device("cuda:0")
    med = lambda v: float(np.median(v))                            # noqa: E731
    res = {"device": torch.cuda.get_device_name(0), "repeats": a.repeats, "tol": TOL, "fp32_mfma_peak_flops": PEAK,
           "library_sha256": hashlib.sha256(open(_lib.lib_path(), "rb").read()).hexdigest(), "rows": []}
    for shape in a.shapes.split(","):
        N, H, B = (int(v) for v in shape.split("x"))
        net = model(N, H, dev)
        y0 = torch.rand((B, N), device=dev, generator=torch.Generator(dev).manual_seed(N))
        with torch.no_grad():
            P = engine.params_cached(*params_of(net))
            free = (P.g > 0).reshape(1, -1).repeat(B, 1)
            m = free.float() * 0.5
            r = engine.steady_residual(P, y0)[1]
            k_ms = med(timed(lambda: engine.reduced_jacobian(P, y0, m, r), a.repeats))
            first = pa.steady_states(net, y0, tol=TOL)
            steps = int(first.iterations.max())
            s_ms = med(timed(lambda: pa.steady_states(net, y0, tol=TOL, max_iter=steps), a.repeats))
            got = pa.steady_states(net, y0, tol=TOL, max_iter=steps)
            e_ms = med(timed(lambda: einsum_iteration(net, y0, free, steps), a.repeats, warmup=1))
            ye, rhoe = einsum_iteration(net, y0, free, steps)
            target = max(float(got.residual.max()), TOL)
            T, o_ms, rhoT = 15.0, None, None
            while True:
                t = torch.tensor([0.0, T], dtype=torch.float64, device=dev)
                yT = pa.odeint(net, y0, t, method="dopri5")[-1]
                rhoT = float(torch.where(free, engine.steady_residual(P, yT)[1].abs(), 0.0).amax())
                if rhoT <= target or T >= 240:
                    o_ms = med(timed(lambda: pa.odeint(net, y0, t, method="dopri5"), max(1, a.repeats // 2), warmup=0))
                    break
                T *= 2
        flops = 8.0 * H * H * N * B
        row = {"N": N, "H": H, "B": B, "statuses": first.status.tolist(), "steps": steps,
               "reduced_jacobian_ms": k_ms, "reduced_jacobian_flops": flops, "reduced_jacobian_fraction_of_peak": flops / (k_ms * 1e-3) / PEAK,
               "steady_states_ms": s_ms, "ms_per_iteration": s_ms / max(1, steps), "residual": float(got.residual.max()),
               "einsum_iteration_ms": e_ms, "einsum_over_steady_states": e_ms / s_ms, "einsum_residual": float(rhoe.max()),
               "einsum_distance": float((ye - got.y).abs().max()),
               "odeint_T": T, "odeint_ms": o_ms, "odeint_residual": rhoT, "odeint_reached_the_residual": rhoT <= target,
               "odeint_over_steady_states": o_ms / s_ms, "odeint_distance": float((yT - got.y).abs().max())}
        print(json.dumps(row))
        res["rows"].append(row)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
    print("wrote", a.out)


if __name__ == "__main__":
    main()
