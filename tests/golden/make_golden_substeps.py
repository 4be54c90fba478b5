#!/usr/bin/env python3
"""Generate G17, the fixture of `options={"step_size": h}` on the fixed-grid methods (solvers.py:36-103).

Like make_goldens.py it runs only where the reference is mounted: it imports the reference's own ODENet, odeint and
odeint_adjoint, runs them on G3's problem with a step size and stores inputs, outputs and gradients -- data only.
Re-run with:  PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_substeps.py

Keys of g17_substeps.npz (method in euler / midpoint / rk4, grid in t2 / t5 / t_dec, y0 in single / batch, h as
repr(float)):
    p_*, y0_single, y0_batch, t2, t5, t5_64, t_dec, hs        the inputs (G3's)
    G/<grid>/<y0>                                             cotangent of the solution (randn, seed 13)
    <method>/<grid>/<h>/<y0>/sol, grad_y0, grad_Ws ... grad_g  odeint solution; odeint_adjoint gradients of sum(G * sol)
    nsteps/<grid>/<h>            forward grid steps, len(grid) - 1 of the reference's _grid_constructor_from_step_size
    nsteps_bwd/<grid>/<h>        the same for every interval of the backward solve, in the order it visits them
    adjstep/*                    rk4, t5, batch, forward h = 0.5, adjoint_options={"step_size": 0.25}
    f64/<method>/sol             float64 t (t5_64), h = 0.07, batch, forward only;  nsteps/t5_64/0.07
    ps/*                         per-sample grids t [5, 2], h = 0.25, rk4: the reference's loop over samples
    truth64/<y0>                 t5: the reference's dopri5 in float64, rtol 1e-10, atol 1e-12
"""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import make_goldens as mg  # noqa: E402  (sets the reference path; its generators run under __main__ only)

import numpy as np  # noqa: E402
import torch  # noqa: E402
from torchdiffeq import odeint, odeint_adjoint  # noqa: E402  (reference)
from torchdiffeq._impl.solvers import FixedGridODESolver  # noqa: E402

HS = (0.5, 0.75, 0.125, 0.3)
METHODS = ("euler", "midpoint", "rk4")


def nsteps_of(t, h):
    return len(FixedGridODESolver._grid_constructor_from_step_size(h)(None, None, t)) - 1


def nsteps_bwd(t, h):
    """grid steps of the backward solve's odeint calls, interval [t[i], t[i-1]] for i = T-1 .. 1 (adjoint.py:137-154);
    a decreasing pair is integrated in reversed time (misc.py:210-212)"""
    out = []
    for i in range(len(t) - 1, 0, -1):
        pair = t[i - 1:i + 1].flip(0)
        out.append(nsteps_of(-pair if pair[0] > pair[1] else pair, h))
    return np.asarray(out, dtype=np.int64)


def run_adjoint(net, y0, t, method, G, h, adjoint_options=None):
    for p in net.parameters():
        p.grad = None
    y0 = y0.clone().requires_grad_(True)
    sol = odeint_adjoint(net, y0, t, method=method, options={"step_size": h}, adjoint_options=adjoint_options)
    (sol * G).sum().backward()
    return sol.detach().numpy(), y0.grad.numpy().copy(), mg.grads_np(net)


def main():
    out = {}
    N, H = 40, 6
    net = mg.make_net(N, H, seed=3, dense_std=0.12, neg_g_frac=0.15)
    out.update(mg.pfx(mg.params_np(net), "p_"))
    torch.manual_seed(7)
    y0_single = torch.rand(1, N)
    y0_batch = torch.rand(5, 1, N) * 1.5 - 0.25
    t2 = torch.tensor([0.0, 2.0])
    t5 = torch.tensor([0.0, 2.0, 3.0, 7.0, 9.0])
    t5_64 = t5.double() * 0.1 + 0.013
    t_dec = torch.tensor([1.0, 0.6, 0.1])
    grids = (("t2", t2), ("t5", t5), ("t_dec", t_dec))
    y0s = (("single", y0_single), ("batch", y0_batch))
    out.update(y0_single=y0_single.numpy(), y0_batch=y0_batch.numpy(), t2=t2.numpy(), t5=t5.numpy(),
               t5_64=t5_64.numpy(), t_dec=t_dec.numpy(), hs=np.asarray(HS))
    Gs = {}
    for tname, t in grids:
        for yname, y0 in y0s:
            torch.manual_seed(13)
            Gs[tname, yname] = torch.randn((len(t),) + tuple(y0.shape))
            out["G/%s/%s" % (tname, yname)] = Gs[tname, yname].numpy()
        for h in HS:
            fwd = -t if t[0] > t[1] else t
            out["nsteps/%s/%r" % (tname, h)] = np.int64(nsteps_of(fwd, h))
            out["nsteps_bwd/%s/%r" % (tname, h)] = nsteps_bwd(t, h)
    for method in METHODS:
        for tname, t in grids:
            for h in HS:
                for yname, y0 in y0s:
                    key = "%s/%s/%r/%s/" % (method, tname, h, yname)
                    with torch.no_grad():
                        sol = odeint(net, y0, t, method=method, options={"step_size": h})
                    s2, gy0, gp = run_adjoint(net, y0, t, method, Gs[tname, yname], h)
                    assert np.array_equal(s2, sol.numpy())
                    out[key + "sol"] = sol.numpy()
                    out[key + "grad_y0"] = gy0
                    out.update(mg.pfx(gp, key))
    # the backward solve with a step of its own
    s2, gy0, gp = run_adjoint(net, y0_batch, t5, "rk4", Gs["t5", "batch"], 0.5, adjoint_options={"step_size": 0.25})
    out.update({"adjstep/sol": s2, "adjstep/grad_y0": gy0, "adjstep/nsteps_bwd": nsteps_bwd(t5, 0.25)})
    out.update(mg.pfx(gp, "adjstep/"))
    # float64 time grid, forward only (as G3)
    for method in METHODS:
        with torch.no_grad():
            out["f64/%s/sol" % method] = odeint(net, y0_batch, t5_64, method=method, options={"step_size": 0.07}).numpy()
    out["nsteps/t5_64/0.07"] = np.int64(nsteps_of(t5_64, 0.07))
    # per-sample grids: the reference's loop over samples, one backward of the summed loss
    tps = torch.stack([torch.tensor([0.1 * b, 0.1 * b + 0.4 + 0.33 * b]) for b in range(5)])
    torch.manual_seed(13)
    Gps = torch.randn(2, 5, 1, N)
    for p in net.parameters():
        p.grad = None
    yb = y0_batch.clone().requires_grad_(True)
    ends = [odeint_adjoint(net, point, time, method="rk4", options={"step_size": 0.25})[1]
            for time, point in zip(tps, yb)]
    end = torch.stack(ends)                                   # [5, 1, N]
    (end * Gps[1]).sum().backward()
    out.update({"ps/t": tps.numpy(), "ps/G": Gps.numpy(), "ps/end": end.detach().numpy(), "ps/grad_y0": yb.grad.numpy().copy(),
                "ps/nsteps": np.asarray([nsteps_of(time, 0.25) for time in tps], dtype=np.int64)})
    out.update(mg.pfx(mg.grads_np(net), "ps/"))
    # what the option is for: the converged solution on t5
    net64 = mg.make_net(N, H, seed=3, dense_std=0.12, neg_g_frac=0.15).double()
    for yname, y0 in y0s:
        with torch.no_grad():
            out["truth64/" + yname] = odeint(net64, y0.double(), t5.double(), method="dopri5", rtol=1e-10, atol=1e-12).numpy()
    mg.save("g17_substeps", **out)


if __name__ == "__main__":
    main()
