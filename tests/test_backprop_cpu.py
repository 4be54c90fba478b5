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
       "phx_debug_backprop_launches", "phx_debug_backprop_plan")


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


def bp_plan(N, H, B, T=5, method="rk4", cus=256):
    """phx_debug_backprop_plan as a dict (None: no plan); cus = 256 needs no device"""
    from phoenix_amd import _lib
    plan = (C.c_int * 8)()
    if _lib.load().phx_debug_backprop_plan(cus, N, H, B, T, _lib.METHODS[method], plan) == 0:
        assert list(plan) == [0] * 8
        return None
    return dict(zip(("HT", "NB", "G", "TG", "ntg", "nblk", "chunk_rows", "launches"), plan))


# the launch geometries tests/test_backprop_geometry_gpu.py is there for, on the 256 CUs of an MI355X
GEOMETRY = {
    "g1": ((32, 6, 5), dict(HT=3, NB=1, G=1, TG=1, ntg=1, nblk=1, launches=1)),
    "g17": ((530, 12, 5), dict(HT=3, NB=1, G=17, TG=1, ntg=1, nblk=17, launches=1)),
    "g35": ((1100, 12, 20), dict(HT=3, NB=1, G=35, TG=1, ntg=2, nblk=35, launches=1)),
    "nb2": ((350, 40, 1530), dict(HT=3, NB=2, G=6, TG=24, ntg=4, nblk=11, launches=1)),
    "nbmax": ((1000, 34, 4096), dict(HT=3, NB=8, G=4, TG=64, ntg=4, nblk=32, launches=1)),      # H = 34: the widest with NB = 8
    "nb4x2": ((1000, 40, 4096), dict(HT=3, NB=4, G=8, TG=32, ntg=4, nblk=32, chunk_rows=2048, launches=2)),
    "nb_ht8": ((350, 100, 1530), dict(HT=8, NB=2, G=6, TG=24, ntg=4, nblk=11, launches=1)),
    "pad": ((200, 100, 70), dict(HT=8, NB=1, G=7, TG=2, ntg=4, nblk=7, launches=1)),
    "b4136": ((350, 40, 4096 + 40), dict(HT=3, NB=4, G=3, TG=65, ntg=4, nblk=11, launches=1)),   # last group: 40 rows
    "chunk": ((700, 40, 4096 + 40), dict(HT=3, NB=6, G=4, TG=64, ntg=4, nblk=22, chunk_rows=4096, launches=2)),
    "chunk_tail": ((700, 40, 40), dict(HT=3, NB=1, G=22, TG=1, ntg=3, nblk=22, launches=1)),
}


def test_backprop_plan_on_256_cus(monkeypatch):
    """phx_debug_backprop_plan with cus = 256 given (no device): the geometry of every case of the GPU file, the planner's
    invariants over seeded random shapes, and the calls without a plan"""
    for name, ((N, H, B), want) in sorted(GEOMETRY.items()):
        got = bp_plan(N, H, B)
        assert got is not None, name
        assert {k: got[k] for k in want} == want, (name, got)
    # nb_ht8: the smallest multiple of 64 minus 6 whose plan keeps two gene blocks per workgroup at H = 100
    (N, H, B), _ = GEOMETRY["nb_ht8"]
    assert B % 64 == 58
    for b in range(58, B, 64):
        assert bp_plan(N, H, b)["NB"] == 1, b
    r = np.random.RandomState(20)
    for _ in range(200):
        N, H, B = int(r.randint(1, 3001)), int(r.randint(1, 129)), int(r.randint(1, 8193))
        d = bp_plan(N, H, B)
        assert d is not None, (N, H, B)                  # a chunk of 16 rows needs ceil(N / 32) <= 94 workgroups
        ntt = -(-min(B, d["chunk_rows"]) // 16)          # trajectory tiles of the first launch
        assert d["HT"] == (3 if H <= 48 else 8) and d["nblk"] == -(-N // 32) and 1 <= d["NB"] <= 8, (N, H, B, d)
        assert d["TG"] * d["G"] <= 256, (N, H, B, d)
        assert d["NB"] * d["G"] >= d["nblk"] > (d["G"] - 1) * d["NB"], (N, H, B, d)
        assert d["TG"] == -(-ntt // 4) and d["ntg"] == (ntt if d["TG"] == 1 else 4), (N, H, B, d)
        assert d["launches"] == -(-B // d["chunk_rows"]), (N, H, B, d)
        assert d["chunk_rows"] == B or d["chunk_rows"] in (4096, 2048, 1024, 512, 256, 128, 64, 32, 16), (N, H, B, d)
    assert bp_plan(350, 40, 64, method="dopri5") is None
    assert bp_plan(350, 129, 64) is None and bp_plan(350, 128, 64) is not None
    assert bp_plan(0, 40, 64) is None and bp_plan(350, 40, 0) is None
    assert bp_plan(350, 40, 1024, method="euler") == bp_plan(350, 40, 1024, method="midpoint") == bp_plan(350, 40, 1024)
    monkeypatch.setenv("PHX_ENGINE", "v0")               # the forced VALU engine (read whenever the planner runs)
    assert bp_plan(350, 40, 64) is None


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
