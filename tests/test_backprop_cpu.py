"""CPU-only checks of the backward pass of `odeint` with a fixed-grid method (backpropagation through the steps): the
C boundary without a device, and the torch arbiter of tests/test_backprop_gpu.py pinned to the reference (G18)."""
import ctypes as C
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch

from conftest import load_golden, relerr, sub

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KEYS = ("Ws", "bs", "Wp", "bp", "Wa", "g")
NEW = ("phx_odeint_backprop_backward", "phx_odeint_backprop_workspace_bytes", "phx_debug_backprop_kernel_m",
       "phx_debug_backprop_launches")


def test_new_exports_in_header_and_binding():
    from phoenix_amd import _lib
    header = open(os.path.join(ROOT, "include", "phoenix_hip.h")).read()
    lib = _lib.load()
    for name in NEW:
        assert re.search(r"\b%s\s*\(" % name, header), name
        assert name in _lib.EXPORTS, name
        assert hasattr(lib, name), name


def test_abi_version_stays_7():
    from phoenix_amd import _lib
    assert _lib.load().phx_abi_version() == 7
    assert "#define PHX_ABI_VERSION 7" in open(os.path.join(ROOT, "include", "phoenix_hip.h")).read()


def test_bad_arguments_without_a_device():
    from phoenix_amd import _lib
    lib = _lib.load()
    one = C.c_void_p(256)           # never dereferenced: every case below is refused before any device call
    P = _lib.PhxParams(one, one, one, one, one, one, 40, 6, None)
    G = _lib.PhxGrads(one, one, one, one, None, one, 1, one)

    def call(p=P, t=one, B=5, T=5, method="rk4", y=one, gy=one, adj=one, grads=G, st=one, ws=one, step=0.0, K=0):
        o = _lib.PhxSolveOpts(_lib.METHODS[method], _lib.CTRL_PER_TRAJECTORY, 0.0, 0.0, 0, 0, 0, 1, 0)
        return lib.phx_odeint_backprop_backward(C.byref(p) if p else None, t, B, T, C.byref(o), y, gy, adj,
                                                C.byref(grads) if grads else None, st, st, st, ws, 1 << 20, None, step, K)

    BAD = 4
    assert call(method="dopri5") == BAD
    assert call(p=None) == BAD and call(t=None) == BAD and call(y=None) == BAD and call(gy=None) == BAD
    assert call(adj=None) == BAD and call(st=None) == BAD and call(ws=None) == BAD
    assert call(B=0) == BAD and call(B=-3) == BAD and call(T=0) == BAD
    assert call(p=_lib.PhxParams(one, one, one, one, one, one, 0, 6, None)) == BAD
    assert call(grads=_lib.PhxGrads(None, one, one, one, None, one, 1, one)) == BAD
    assert call(step=0.5, K=0) == BAD and call(K=-1) == BAD
    assert lib.phx_odeint_backprop_workspace_bytes(0, 6, 5, 5, 0) == 0
    assert lib.phx_odeint_backprop_workspace_bytes(40, 6, 5, 5, -1) == 0


@pytest.mark.parametrize("N, H, B", [(40, 6, 5), (350, 40, 1024), (200, 100, 37)])
def test_workspace_bytes_formula(N, H, B):
    """bytes(K) = bytes(0) + 256 * ceil(K * Bc * N * 4 / 256), Bc = B for a batch that is one launch"""
    from phoenix_amd import _lib
    lib = _lib.load()
    base = lib.phx_odeint_backprop_workspace_bytes(N, H, B, 5, 0)
    assert base > 0
    prev = base
    for K in (1, 2, 7, 100, 1001):
        got = lib.phx_odeint_backprop_workspace_bytes(N, H, B, 5, K)
        assert got == base + 256 * -(-(K * B * N * 4) // 256), (K, got)
        assert got > prev
        prev = got
    assert lib.phx_odeint_backprop_workspace_bytes(N, 200, B, 5, 3) == 0      # H > 128: no kernel plans the shape


class TorchNet(torch.nn.Module):
    """plain-torch restatement of ODENet.forward (odenet.py:85-91), the arbiter of tests/test_backprop_gpu.py"""

    def __init__(self, p, dtype):
        super().__init__()
        for k in KEYS:
            setattr(self, k, torch.nn.Parameter(torch.from_numpy(p[k]).to(dtype)))

    def forward(self, t, y):
        s = y - 0.5
        a = s / (1 + s.abs())
        sums = a @ self.Ws.t() + self.bs
        prods = torch.exp(torch.log1p(a) @ self.Wp.t() + self.bp)
        joint = torch.cat((sums, prods), dim=-1) @ self.Wa.t()
        return torch.relu(self.g) * (joint - y)


@pytest.mark.parametrize("h", [0.5, 0.75, 0.125, 0.3, None])
@pytest.mark.parametrize("tname", ["t2", "t5", "t_dec"])
@pytest.mark.parametrize("method", ["euler", "midpoint", "rk4"])
def test_torch_arbiter_reproduces_g18(method, tname, h):
    from phoenix_amd import generic
    g18 = load_golden("g18_backprop")
    p = sub(g18, "p_")
    p = dict(p, g=p["g"].reshape(1, -1))
    for yname in ("single", "batch"):
        c = sub(g18, "%s/%s/%s/%s/" % (method, tname, "none" if h is None else repr(h), yname))
        net = TorchNet(p, torch.float32)
        y0 = torch.from_numpy(g18["y0_" + yname]).requires_grad_(True)
        sol = generic.integrate(net, y0, torch.from_numpy(g18[tname]), 1e-7, 1e-9, method, step_size=h)
        (sol * torch.from_numpy(g18["G/%s/%s" % (tname, yname)])).sum().backward()
        assert relerr(sol.detach().numpy(), c["sol"]) < 1e-5
        assert relerr(y0.grad.numpy(), c["grad_y0"]) < 1e-5
        for k in KEYS:
            assert relerr(getattr(net, k).grad.numpy().reshape(c["grad_" + k].shape), c["grad_" + k]) < 1e-5, k


def test_store_hazard_check_covers_the_new_listing():
    from phoenix_amd import build
    build.build()
    src = os.path.join(build.CSRC, "phx_bp.hip")
    assert "phx_bp.hip" in build.LISTINGS and os.path.exists(build.listing_of(src))
    text = open(build.listing_of(src)).read()
    assert "k1_solve_bp" in text
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "check_store_hazard.py"), build.listing_of(src)],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    assert re.search(r": [1-9]\d* wide stores", r.stdout), r.stdout
