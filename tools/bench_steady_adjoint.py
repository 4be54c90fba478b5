#!/usr/bin/env python3
"""The implicit adjoint of `steady_states(differentiable=True)` against what a caller had before it (run on the MI355X):
    python tools/bench_steady_adjoint.py [--shapes 11165x40x60,14691x200x24] [--knockouts 64] [--repeats 5]
                                         [--out profiles/steady_adjoint.json]
Per shape (N, H, states), on the model and the states of tools/bench_steady.py: `knockouts` x states rows, row k * states + s
being state s with gene k set to 0 and held (a row-wise clamp), relaxed by `steady_states(differentiable=True)`;
L = sum(y* G) over the converged rows, G Gaussian.
  - phx_steady_param_grads alone on the backward pass's own lam, q, hid, and what share of the 157.3 TFLOP/s fp32 MFMA
    peak its 2 B N (4H + 2) flops come to;
  - the whole backward pass (autograd.grad of L to the six parameter tensors and y0), and the forward solve beside it;
  - (a) the same adjoint with torch: S and C^T q by `torch.einsum` / matmul in blocks of rows, `torch.linalg.solve` in
    float64, the parameter gradients by `engine.rhs_vjp` with cot = lam / relu(g);
  - (b) forward plus backward of `odeint_adjoint` (dopri5, per-trajectory control, the same row-wise clamp) to the T at which
    tools/bench_steady.py reached the residual of `steady_states` (--odeint-T, 120 in profiles/steady_states.json).
Warm-up, HIP events, median of the repeats ((b): one run after none, it is seconds long).  The parts run in the order of
--parts, every shape through one part before the next part starts; a line is printed after every figure and the JSON file is
rewritten after every part, so a run that is cut short keeps what it had.  A figure that could not be taken is the string
"not measured" with the reason beside it.  Reads nothing outside the tree; writes one JSON file."""
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

EINSUM_BYTES = 32 << 20  # baseline (a) works in blocks of rows whose float64 systems take this much (128 rows at H = 40, 52 at
#                          H = 200, where hipblasDgetrfBatched could not allocate for 128): its [rows, H, N] intermediates stay small


def einsum_adjoint(net, P, y, free, gy):
    """baseline (a) -> (gy0, Grads)"""
    ws, bs, wp, bp, wa, g = (x.detach() for x in params_of(net))
    H = ws.shape[0]
    eye = torch.eye(2 * H, device=y.device, dtype=torch.float64)
    m = free.float()
    lam, gy0 = torch.empty_like(y), torch.empty_like(y)
    rows = max(1, min(128, EINSUM_BYTES // (32 * H * H)))
    for b0 in range(0, y.shape[0], rows):
        sl = slice(b0, b0 + rows)
        s = y[sl] - 0.5
        d = 1 + s.abs()
        a = s / d
        da = 1 / (d * d)
        dl = da / (1 + a)
        v = torch.exp(torch.log1p(a) @ wp.t() + bp)
        S = torch.cat([torch.einsum("jn,bn,nc->bjc", ws, da * m[sl], wa),
                       v.unsqueeze(2) * torch.einsum("jn,bn,nc->bjc", wp, dl * m[sl], wa)], dim=1)
        b = (m[sl] * gy[sl]) @ wa
        q = torch.linalg.solve(eye - S.transpose(1, 2).double(), b.double()).float()
        u = gy[sl] + da * (q[:, :H] @ ws) + dl * ((q[:, H:] * v) @ wp)
        lam[sl] = m[sl] * u
        gy0[sl] = (1 - m[sl]) * u
    gpos = torch.relu(g).reshape(1, -1)
    cot = torch.where(free, lam / torch.where(gpos > 0, gpos, torch.ones_like(gpos)), torch.zeros_like(lam))
    return gy0, engine.rhs_vjp(P, y, cot, want_vjp_y=False)[1]


def say(*what):
    print(*what, flush=True)


class Case:
    """one shape: the model, the knockout rows, their steady states with a gradient, and the loss"""

    def __init__(self, shape, K, dev):
        self.N, self.H, self.states = (int(v) for v in shape.split("x"))
        N, states = self.N, self.states
        self.B = B = K * states
        self.net = model(N, self.H, dev)
        self.tensors = params_of(self.net)
        y0 = torch.rand((states, N), device=dev, generator=torch.Generator(dev).manual_seed(N))
        start = y0.unsqueeze(0).repeat(K, 1, 1)
        for k in range(K):
            start[k, :, k] = 0.0
        self.start = start.reshape(B, N).requires_grad_(True)
        self.clamp = [(k,) for k in range(K) for _ in range(states)]
        self.G = torch.randn((B, N), device=dev, generator=torch.Generator(dev).manual_seed(N + 1))
        self.wrt = list(self.tensors[:5]) + [self.start]
        self.row = {"N": N, "H": self.H, "states": states, "knockouts": K, "B": B}
        say("case", self.row)
        self.steps = int(pa.steady_states(self.net, self.start, clamp=self.clamp, tol=TOL, max_iter=16).iterations.max())
        self.out = self.forward()
        self.mask = (self.out.status == 0).unsqueeze(1)
        self.loss = torch.where(self.mask, self.out.y * self.G, torch.zeros_like(self.G)).sum()
        self.row.update(steps=self.steps, converged_rows=int((self.out.status == 0).sum()), residual=float(self.out.residual.max()))
        say("  steps", self.steps, "converged rows", self.row["converged_rows"])
        with torch.no_grad():
            self.P = engine.params_cached(*self.tensors)
            self.free = (self.P.g > 0).reshape(1, -1).repeat(B, 1)
            self.free[torch.arange(B, device=dev), torch.tensor([c[0] for c in self.clamp], device=dev)] = False
            self.gy = torch.where(self.mask, self.G, torch.zeros_like(self.G))

    def forward(self):       # (every pass costs the same whether a row is still moving or frozen: the steps the slowest row needs)
        return pa.steady_states(self.net, self.start, clamp=self.clamp, tol=TOL, max_iter=self.steps, differentiable=True)

    def backward(self):
        return torch.autograd.grad(self.loss, self.wrt, retain_graph=True)

    def put(self, **kw):
        self.row.update(kw)
        say("  " + json.dumps(kw))


def part_ours(c, repeats):
    med = lambda v: float(np.median(v))                            # noqa: E731
    c.put(backward_ms=med(timed(c.backward, repeats)))
    c.put(rows_used_by_backward=int((pa.last_backward_info() == 0).sum()))
    c.put(forward_ms=med(timed(c.forward, repeats, warmup=1)))
    # the kernel alone, on the quantities of that backward pass (the chain of steady._SteadyFn.backward, by hand)
    with torch.no_grad():
        P, y, free, gy, B = c.P, c.out.y.detach(), c.free, c.gy, c.B
        step = pa.steady._block_rows(P)
        lams, qs, hids = [], [], []
        for b0 in range(0, B, step):
            sl = slice(b0, b0 + step)
            S, _, hid = engine.reduced_jacobian(P, y[sl], free[sl].float())
            q = engine.steady_solve(S.transpose(1, 2).contiguous(), engine.steady_adjoint_project(P, free[sl].float(), gy[sl]))[0]
            lams.append(engine.steady_adjoint_back(P, y[sl], free[sl].float(), gy[sl], q, hid)[0])
            qs.append(q)
            hids.append(hid)
        lam, q, hid = torch.cat(lams), torch.cat(qs), torch.cat(hids)
        m0, S0 = free[:step].float(), engine.reduced_jacobian(P, y[:step], free[:step].float())[0]
        k_ms = med(timed(lambda: engine.steady_param_grads(P, y, lam, q, hid), repeats))
        flops = 2.0 * B * c.N * (4 * c.H + 2)
        c.put(param_grads_ms=k_ms, param_grads_flops=flops, param_grads_fraction_of_peak=flops / (k_ms * 1e-3) / PEAK,
              backward_block_rows=min(step, B))
        for name, fn in (("project", lambda: engine.steady_adjoint_project(P, m0, gy[:step])),
                         ("reduced_jacobian", lambda: engine.reduced_jacobian(P, y[:step], m0)),
                         ("transposed_solve", lambda: engine.steady_solve(S0, q[:step])),
                         ("back", lambda: engine.steady_adjoint_back(P, y[:step], m0, gy[:step], q[:step], hid[:step]))):
            c.put(**{name + "_ms_per_block": med(timed(fn, repeats))})


def part_einsum(c, repeats):
    with torch.no_grad():
        y = c.out.y.detach()
        e_ms = float(np.median(timed(lambda: einsum_adjoint(c.net, c.P, y, c.free, c.gy), max(1, repeats // 2), warmup=1)))
        c.put(einsum_adjoint_ms=e_ms)
        gy0_e, grads_e = einsum_adjoint(c.net, c.P, y, c.free, c.gy)
    ours = c.backward()
    names = ("Ws", "bs", "Wp", "bp", "Wa")
    c.put(einsum_distance={k: float((getattr(grads_e, k) - o).abs().max()) for k, o in zip(names, ours)},
          largest_gradient={k: float(o.abs().max()) for k, o in zip(names, ours)},
          einsum_distance_y0=float((gy0_e - ours[5]).abs().max()), largest_gradient_y0=float(ours[5].abs().max()))


def part_odeint(c, T):
    t = torch.tensor([0.0, T], dtype=torch.float64, device=c.start.device)
    a, b, e = (torch.cuda.Event(enable_timing=True) for _ in range(3))
    a.record()
    yT = pa.odeint_adjoint(c.net, c.start, t, method="dopri5", clamp=c.clamp, options={"batch_control": "per_trajectory"})[-1]
    b.record()
    b.synchronize()
    c.put(odeint_adjoint_T=T, odeint_adjoint_forward_ms=a.elapsed_time(b))
    torch.autograd.grad((yT.reshape(c.B, c.N) * c.G).sum(), c.wrt)
    e.record()
    e.synchronize()
    with torch.no_grad():
        yT = yT.detach().reshape(c.B, c.N)
        rhoT = float(torch.where(c.free, engine.steady_residual(c.P, yT)[1].abs(), torch.zeros_like(yT)).amax())
    c.put(odeint_adjoint_forward_backward_ms=a.elapsed_time(e), odeint_residual=rhoT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="11165x40x60,14691x200x24")
    ap.add_argument("--knockouts", type=int, default=64)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--odeint-T", type=float, default=120.0)
    ap.add_argument("--parts", default="ours,einsum,odeint")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "steady_adjoint.json"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("bench_steady_adjoint.py measures on the GPU; none is visible")
    dev = torch.device("cuda:0")
    res = {"device": torch.cuda.get_device_name(0), "repeats": a.repeats, "tol": TOL, "fp32_mfma_peak_flops": PEAK,
           "knockouts": a.knockouts, "library_sha256": hashlib.sha256(open(_lib.lib_path(), "rb").read()).hexdigest(), "rows": []}
    cases = [Case(shape, a.knockouts, dev) for shape in a.shapes.split(",")]
    res["rows"] = [c.row for c in cases]
    for c in cases:
        c.row.update(backward_ms="not measured", param_grads_ms="not measured", einsum_adjoint_ms="not measured",
                     odeint_adjoint_forward_backward_ms="not measured")
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    for part in a.parts.split(","):
        for c in cases:
            say("part", part, (c.N, c.H, c.B))
            try:
                {"ours": lambda: part_ours(c, a.repeats), "einsum": lambda: part_einsum(c, a.repeats),
                 "odeint": lambda: part_odeint(c, a.odeint_T)}[part]()
            except Exception as e:                                  # noqa: BLE001
                c.put(**{part + "_reason": repr(e)[:300]})
            with open(a.out, "w") as f:
                json.dump(res, f, indent=1)
    say("wrote", a.out)


if __name__ == "__main__":
    main()
