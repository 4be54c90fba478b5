#!/usr/bin/env python3
"""Generate G18, the fixture of backpropagation through the fixed-grid steps: the reference's own `odeint` (NOT the
adjoint) on the reference's own ODENet, differentiated by `.backward()` (torchdiffeq/_impl/odeint.py:30-74).

Like make_golden_substeps.py it runs only where the reference is mounted, on the CPU, and is never imported by a test.
G17's parameters, initial states, grids and cotangents; data only.
Re-run with:  PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_backprop.py

Keys of g18_backprop.npz (method in euler / midpoint / rk4, grid in t2 / t5 / t_dec, y0 in single / batch, h as
repr(float) or "none" for no step size):
    p_*, y0_single, y0_batch, t2, t5, t_dec, hs               the inputs (G17's)
    G/<grid>/<y0>                                             cotangent of the solution (randn, seed 13: G17's)
    <method>/<grid>/<h>/<y0>/sol, grad_y0, grad_Ws ... grad_g  float32: odeint solution, gradients of sum(G * sol)
    <method>/<grid>/<h>/<y0>/sol64, grad64_y0, grad64_Ws ...   the same run in float64 -- in g18_backprop_f64.npz, rounded
                                                               to float32 for storage (a committed file stays under 1 MiB)
    <method>/<grid>/<h>/<y0>/spread                            max over the seven gradients of relerr(float32, float64)
    ps/*                         per-sample grids t [5, 2], rk4, h = 0.25 (ps/h/*) and no step size (ps/none/*): the
                                 reference's loop over samples (train_insilico.py:128-130), one backward of the summed loss
"""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import make_goldens as mg  # noqa: E402  (sets the reference path; its generators run under __main__ only)

import numpy as np  # noqa: E402
import torch  # noqa: E402
from torchdiffeq import odeint  # noqa: E402  (reference)

HS = (0.5, 0.75, 0.125, 0.3)
METHODS = ("euler", "midpoint", "rk4")
KEYS = ("Ws", "bs", "Wp", "bp", "Wa", "g")


def relerr(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return float(np.max(np.abs(a - b))) / max(float(np.max(np.abs(b))), 1e-30)


def run(net, y0, t, method, G, h):
    """solution and gradients of sum(G * odeint(...)) by backpropagation through the solver, in the dtype of `net`"""
    for p in net.parameters():
        p.grad = None
    dt = next(net.parameters()).dtype
    y0 = y0.to(dt).clone().requires_grad_(True)
    sol = odeint(net, y0, t.to(dt), method=method, options=None if h is None else {"step_size": h})
    (sol * G.to(dt)).sum().backward()
    return sol.detach().numpy(), y0.grad.numpy().copy(), mg.grads_np(net)


def run_per_sample(net, yb, tps, G, h):
    for p in net.parameters():
        p.grad = None
    dt = next(net.parameters()).dtype
    yb = yb.to(dt).clone().requires_grad_(True)
    ends = [odeint(net, point, time.to(dt), method="rk4", options=None if h is None else {"step_size": h})[1]
            for time, point in zip(tps, yb)]
    end = torch.stack(ends)                                   # [5, 1, N]
    (end * G.to(dt)).sum().backward()
    return end.detach().numpy(), yb.grad.numpy().copy(), mg.grads_np(net)


def both(out, key, fn):
    """runs fn(net) in float32 and float64 and stores both with the spread of the gradients"""
    sol, gy0, gp = fn(both.net32)
    sol64, gy064, gp64 = fn(both.net64)
    out[key + "sol"] = sol
    out[key + "grad_y0"] = gy0
    out.update(mg.pfx(gp, key))
    out[key + "sol64"] = sol64
    out[key + "grad64_y0"] = gy064
    out.update({key + "grad64_" + k: gp64["grad_" + k] for k in KEYS})
    spread = max([relerr(gy0, gy064)] + [relerr(gp["grad_" + k], gp64["grad_" + k]) for k in KEYS])
    out[key + "spread"] = np.float64(spread)
    return spread


def main():
    out = {}
    N, H = 40, 6
    both.net32 = mg.make_net(N, H, seed=3, dense_std=0.12, neg_g_frac=0.15)
    both.net64 = mg.make_net(N, H, seed=3, dense_std=0.12, neg_g_frac=0.15).double()
    out.update(mg.pfx(mg.params_np(both.net32), "p_"))
    torch.manual_seed(7)
    y0_single = torch.rand(1, N)
    y0_batch = torch.rand(5, 1, N) * 1.5 - 0.25
    t2 = torch.tensor([0.0, 2.0])
    t5 = torch.tensor([0.0, 2.0, 3.0, 7.0, 9.0])
    t_dec = torch.tensor([1.0, 0.6, 0.1])
    grids = (("t2", t2), ("t5", t5), ("t_dec", t_dec))
    y0s = (("single", y0_single), ("batch", y0_batch))
    out.update(y0_single=y0_single.numpy(), y0_batch=y0_batch.numpy(), t2=t2.numpy(), t5=t5.numpy(), t_dec=t_dec.numpy(),
               hs=np.asarray(HS))
    Gs = {}
    for tname, t in grids:
        for yname, y0 in y0s:
            torch.manual_seed(13)
            Gs[tname, yname] = torch.randn((len(t),) + tuple(y0.shape))
            out["G/%s/%s" % (tname, yname)] = Gs[tname, yname].numpy()
    worst = 0.0
    for method in METHODS:
        for tname, t in grids:
            for h in HS + (None,):
                for yname, y0 in y0s:
                    key = "%s/%s/%s/%s/" % (method, tname, "none" if h is None else repr(h), yname)
                    s = both(out, key, lambda net: run(net, y0, t, method, Gs[tname, yname], h))
                    worst = max(worst, s)
                    if s > 5e-6:
                        print("spread %.2e  %s" % (s, key))
    tps = torch.stack([torch.tensor([0.1 * b, 0.1 * b + 0.4 + 0.33 * b]) for b in range(5)])
    torch.manual_seed(13)
    Gps = torch.randn(2, 5, 1, N)
    out.update({"ps/t": tps.numpy(), "ps/G": Gps.numpy()})
    for name, h in (("h", 0.25), ("none", None)):
        worst = max(worst, both(out, "ps/%s/" % name, lambda net: run_per_sample(net, y0_batch, tps, Gps[1], h)))
    print("largest spread %.2e" % worst)
    is64 = lambda k: k.rsplit("/", 1)[-1].startswith(("sol64", "grad64_"))      # noqa: E731
    mg.save("g18_backprop", **{k: v for k, v in out.items() if not is64(k)})
    mg.save("g18_backprop_f64", **{k: np.asarray(v, np.float32) for k, v in out.items() if is64(k)})


if __name__ == "__main__":
    main()
