#!/usr/bin/env python3
"""Generate G25: an fp64 truth for every dopri5 kernel family, and the reference's own distance from it.

Like the other make_golden_*.py scripts it runs only where the reference is mounted, on the CPU, and is never imported by
a test.  For every case of tests/g25.py (the shapes that reach fwd3 / adj3 and every hidden-chunk count of fwd3c / adj3c)
it runs the reference's `odeint_adjoint` on the reference's own ODENet carrying g25.params():
  * in float64 at a tight tolerance: the truth.  A second run at ten times that tolerance says how converged it is.
  * in float32 at rtol x {0.85 ... 1.15}, atol 1e-9 (the reference's defaults, jittered as in G12): once as one batched
    call (shared step control) and once as the reference's loop of B calls (per-trajectory control).  Only their errors
    against the truth are kept.
  * the CPU oracle with and without the parameter block in the adjoint norm, the same way: the cost of the block the
    engine's controllers leave out, measured on the CPU, for the bar of tests/g25.py.
Data only; about 25 minutes on 8 cores at the default tolerance (rtol 1e-13, atol 1e-15).  Re-run with:  PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_truth.py [--tol RTOL] [--jobs J]

Keys (<run> = n<N>_h<H>_b<B>/<mode>/, mode in shared / per / multi as in g25.RUNS):
    truth_rtol, truth_atol          the truth's tolerance (the backward solve's atol times the largest cotangent, if below 1)
    n<N>_h<H>_b<B>/checksums        [6, 2] sum and sum of squares of Ws, bs, Wp, bp, Wa, g
    <run>truth/sol                  [T-1, B, N] the solution after t[0]
    <run>truth/y0, bs, bp, g        dL/dy0 [B, N] and the small gradients in full
    <run>truth/Ws, Wp, Wa, max_*    the weight gradients at g25.positions() and the maximum of each whole tensor
                                    (the positions' values in g25_dopri5_truth_w.npz: a committed file stays under 1 MiB)
    <run>converged                  largest relerr between the truth and the run at ten times its tolerance (< 1e-8)
    <run>ref_err                    [7, 8] errors of the seven float32 reference runs: g25.GRADS and the per-row figure
    <run>ref_sol_err                [7] relerr of their solutions against the truth's
    <run>oracle_err                 [2, 8] the same for the CPU oracle with / without the parameter block in the norm
The arrays are the float64 results rounded to float32 for storage (6e-8 relative, a fiftieth of the smallest error the
reference shows; every stored error is measured against the rounded arrays, as a test measures).  A "per" run of the
training-scale regime has the truth of its "shared" run (the same problem), which is stored once.
"""
import multiprocessing as mp
import os
import sys
import time

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
import make_goldens as mg  # noqa: E402  (sets the reference path; its generators run under __main__ only)

import numpy as np  # noqa: E402
import torch  # noqa: E402
from torchdiffeq import odeint_adjoint  # noqa: E402  (reference)

import g25  # noqa: E402


def ref_net(shape, p, dtype):
    net = mg.make_net(shape[0], shape[1], seed=0)
    with torch.no_grad():
        net.net_sums.linear_out.weight.copy_(torch.from_numpy(p["Ws"]))
        net.net_sums.linear_out.bias.copy_(torch.from_numpy(p["bs"]))
        net.net_prods.linear_out.weight.copy_(torch.from_numpy(p["Wp"]))
        net.net_prods.linear_out.bias.copy_(torch.from_numpy(p["bp"]))
        net.net_alpha_combine.linear_out.weight.copy_(torch.from_numpy(p["Wa"]))
        net.gene_multipliers.copy_(torch.from_numpy(p["g"]).reshape(1, -1))
    return net.double() if dtype == torch.float64 else net.float()


def run(task):
    """one reference run: (shape, mode, kind, rtol, atol) -> (task, solution [T, B, N], g25.stored() gradients)"""
    shape, mode, kind, rtol, atol = task
    torch.set_num_threads(1)
    t0 = time.time()
    N, H, B = shape
    dtype = torch.float32 if kind == "ref" else torch.float64
    p, y0, t, G = g25.inputs(shape, mode)
    net = ref_net(shape, p, dtype)
    for q in net.parameters():
        q.grad = None
    tt = torch.from_numpy(t).to(dtype)
    Gt = torch.from_numpy(G).to(dtype)
    if mode == "per" and kind == "ref":          # the reference's loop, one sample at a time (train_insilico.py:128-130)
        ys = [torch.from_numpy(y0[b:b + 1]).to(dtype).requires_grad_(True) for b in range(B)]
        sols = [odeint_adjoint(net, y, tt, rtol=rtol, atol=atol, method="dopri5") for y in ys]
        sum((s * Gt[:, b:b + 1]).sum() for b, s in enumerate(sols)).backward()
        sol = torch.cat(sols, 1).detach().numpy()
        gy = torch.cat([y.grad for y in ys]).numpy()
    else:                                        # (the truth does not depend on how the steps are controlled)
        y = torch.from_numpy(y0).to(dtype).reshape(B, 1, N).requires_grad_(True)
        # (the adjoint's atol goes with the size of the cotangents: at training scale a fixed one would dominate its tolerance)
        s = odeint_adjoint(net, y, tt, rtol=rtol, atol=atol, method="dopri5",
                           adjoint_atol=atol * min(1.0, float(np.abs(G).max())) if kind != "ref" else None)
        (s * Gt.reshape(-1, B, 1, N)).sum().backward()
        sol = s.detach().numpy().reshape(-1, B, N)
        gy = y.grad.numpy().reshape(B, N)
    gr = {k[len("grad_"):]: v for k, v in mg.grads_np(net).items()}
    gr["y0"] = gy
    print("  %-22s %-6s rtol %.3g  %.0f s" % (g25.name(shape, mode), kind, rtol, time.time() - t0), flush=True)
    return task, sol, g25.stored(shape, gr)


def oracle_errors(shape, mode, truth):
    from oracle import oracle as orc
    orc.build()
    p, y0, t, G = g25.inputs(shape, mode)
    net = orc.Net(*[p[k] for k in g25.KEYS])
    rows = []
    for theta in (True, False):
        if mode == "per":
            tb = np.tile(t[None], (shape[2], 1))
            sol = orc.odeint_per_sample(net, y0, tb, method="dopri5")
            adj, gr = orc.adjoint_backward_per_sample(net, tb, sol, G.transpose(1, 0, 2).copy(), method="dopri5",
                                                      theta_in_norm=theta)
        else:
            sol = orc.odeint(net, y0, t, method="dopri5")
            adj, gr = orc.adjoint_backward(net, t, sol, G, method="dopri5", theta_in_norm=theta)
        e = g25.errors(g25.stored(shape, dict(gr, y0=adj)), truth)
        rows.append([e[k] for k in g25.GRADS + ("row",)])
    return np.array(rows)


def has_own_truth(shape, mode):
    return mode != "per" or g25.regime(shape) == "unit"


def main():
    rtol = float(sys.argv[sys.argv.index("--tol") + 1]) if "--tol" in sys.argv else 1e-13
    jobs = int(sys.argv[sys.argv.index("--jobs") + 1]) if "--jobs" in sys.argv else 8
    atol = rtol * 1e-2
    tasks = []
    for shape, mode in g25.RUNS:
        if has_own_truth(shape, mode):
            tasks += [(shape, mode, "truth", rtol, atol), (shape, mode, "truth10", 10 * rtol, 10 * atol)]
        tasks += [(shape, mode, "ref", 1e-7 * f, 1e-9) for f in g25.JITTER]
    # the longest first: float64 before float32, large before small
    tasks.sort(key=lambda k: -k[0][0] * k[0][1] * k[0][2] * (0.01 if k[2] == "ref" else 30 if g25.regime(k[0]) == "unit" else 1))
    t0 = time.time()
    with mp.Pool(jobs) as pool:
        done = {r[0][:3] + (r[0][3],): r[1:] for r in pool.imap_unordered(run, tasks)}
    print("reference runs: %.0f s" % (time.time() - t0))
    out = {"truth_rtol": np.float64(rtol), "truth_atol": np.float64(atol)}
    big, loose = {}, []
    for shape in g25.SHAPES:
        out["n%d_h%d_b%d/checksums" % shape] = g25.checksums(g25.inputs(shape, "shared")[0])
    for shape, mode in g25.RUNS:
        key = g25.name(shape, mode)
        src = mode if has_own_truth(shape, mode) else "shared"
        sol, full = done[shape, src, "truth", rtol]
        conv = g25.worst(g25.errors(done[shape, src, "truth10", 10 * rtol][1], full))
        out[key + "converged"] = np.float64(conv)
        loose += [(key, conv)] if conv >= 1e-8 else []
        tr = {k: (v if k.startswith("max_") else v.astype(np.float32)) for k, v in full.items()}    # as stored
        if src == mode:
            out[key + "truth/sol"] = sol[1:].astype(np.float32)
            for k, v in tr.items():
                (big if k in g25.WEIGHTS else out)[key + "truth/" + k] = v
        ref = [g25.errors(done[shape, mode, "ref", 1e-7 * f][1], tr) for f in g25.JITTER]
        out[key + "ref_err"] = np.array([[e[k] for k in g25.GRADS + ("row",)] for e in ref])
        out[key + "ref_sol_err"] = np.array([g25._rel(done[shape, mode, "ref", 1e-7 * f][0][1:], sol[1:]) for f in g25.JITTER])
        out[key + "oracle_err"] = oracle_errors(shape, mode, tr)
        w = out[key + "ref_err"][:, :7].max(1)
        o = out[key + "oracle_err"][:, :7].max(1)
        print("%-24s %-5s converged %.1e | reference worst: median %.2e min %.2e max %.2e row %.2e | oracle %.2e, without "
              "theta %.2e (row %.2e / %.2e)" % (key, g25.regime(shape), conv, np.median(w), w.min(), w.max(),
                                                 out[key + "ref_err"][:, 7].max(), o[0], o[1],
                                                 out[key + "oracle_err"][0, 7], out[key + "oracle_err"][1, 7]))
    mg.save("g25_dopri5_truth", **out)
    mg.save("g25_dopri5_truth_w", **big)
    assert not loose, ("the truth is not converged to 1e-8: tighten --tol", loose)


if __name__ == "__main__":
    main()
