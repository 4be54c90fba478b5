#!/usr/bin/env python3
"""Generate G26: the reference's own fixed-grid odeint_adjoint in float64, the anchor of the arbiter of tests/g26.py.

Like the other make_golden_*.py scripts it runs only where the reference is mounted, on the CPU, and is never imported by
a test.  For every case of CASES it runs the reference's `odeint_adjoint` on the reference's own ODENet carrying
g26.params(), everything in float64 (parameters, states, cotangents and the time grid: the step grid of
options["step_size"] is then formed in float64 on both sides), and stores the solution and all seven gradients in full,
in float64.  tests/test_fixed_grid_cpu.py runs the arbiter of tests/g26.py (phoenix_amd.generic on a plain-torch net) on
the same inputs and holds it to these arrays: the same arithmetic in another order.  Data only; a few seconds.
Re-run with:  PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_fixed_truth.py

Keys (<case> = g26.golden_name(case)):
    <case>/checksums                  [6, 2] sum and sum of squares of Ws, bs, Wp, bp, Wa, g (the inputs are drawn by
                                      g26.golden_inputs, never stored)
    <case>/sol                        [T, B, N]
    <case>/grad_y0, grad_Ws ... grad_g
"""
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
import make_goldens as mg  # noqa: E402  (sets the reference path; its generators run under __main__ only)

import numpy as np  # noqa: E402
import torch  # noqa: E402
from torchdiffeq import odeint_adjoint  # noqa: E402  (reference)

import g26  # noqa: E402


def ref_net(N, H, p):
    net = mg.make_net(N, H, seed=0).double()
    with torch.no_grad():
        net.net_sums.linear_out.weight.copy_(torch.from_numpy(p["Ws"]))
        net.net_sums.linear_out.bias.copy_(torch.from_numpy(p["bs"]))
        net.net_prods.linear_out.weight.copy_(torch.from_numpy(p["Wp"]))
        net.net_prods.linear_out.bias.copy_(torch.from_numpy(p["bp"]))
        net.net_alpha_combine.linear_out.weight.copy_(torch.from_numpy(p["Wa"]))
        net.gene_multipliers.copy_(torch.from_numpy(p["g"]).reshape(1, -1))
    return net


def main():
    out = {}
    for case in g26.GOLDEN_CASES:
        (N, H, B), method, tname, h, ah = case
        p, y0, t, G = g26.golden_inputs(case)
        net = ref_net(N, H, p)
        for q in net.parameters():
            q.grad = None
        y = torch.from_numpy(y0).double().reshape(B, 1, N).requires_grad_(True)
        sol = odeint_adjoint(net, y, torch.from_numpy(t), method=method, options={"step_size": h} if h else None,
                             adjoint_options={"step_size": ah} if ah else None)
        assert sol.dtype == torch.float64
        (sol * torch.from_numpy(G).double().reshape(-1, B, 1, N)).sum().backward()
        key = g26.golden_name(case) + "/"
        out[key + "checksums"] = g26.checksums(p)
        out[key + "sol"] = sol.detach().numpy().reshape(-1, B, N)
        out[key + "grad_y0"] = y.grad.numpy().reshape(B, N).copy()
        out.update(mg.pfx(mg.grads_np(net), key))
        print("  %s" % key)
    mg.save("g26_fixed_truth", **out)


if __name__ == "__main__":
    main()
