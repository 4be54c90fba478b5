"""`odeint_calls` with a time grid per call (phx_odeint with opts->calls > 1 and t_per_sample under shared control): K
shared-control calls over K different grids in a few launches, dopri5 on k1_solve_fwd3 / k1_solve_fwd3c.  On the MI355X;
run with `-m gpu`."""
import ctypes as C

import numpy as np
import pytest
import torch

from conftest import relerr
from test_gpu_parity import TOL_DOPRI, make_net, onet_of, rand_params   # the bars of test_odeint_calls_equals_separate_calls

pytestmark = pytest.mark.gpu

TOL_FIXED_CALLS = 5e-6      # test_gpu_parity.py::test_odeint_calls_equals_separate_calls, fixed grids


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "these tests need the MI355X"
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def pa():
    import phoenix_amd
    return phoenix_amd


def _grids(K, T, dtype):
    """K grids of T points that differ in start, span and direction (call 1 decreases)"""
    rows = []
    for k in range(K):
        start, span = 0.3 * k - 0.2, 0.5 + 0.35 * k
        g = start + span * np.linspace(0.0, 1.0, T) ** (1.0 + 0.25 * (k % 3))
        rows.append(g[::-1].copy() if k == 1 else g)
    return np.stack(rows).astype(dtype)


def _y0s(N, B, K):
    rs = np.random.RandomState(K)
    return np.stack([(rs.rand(B, 1, N).astype(np.float32) - 0.5) * (0.2 + 0.9 * k) for k in range(K)])


def _kernel(N, H, B, T, K, method):
    from phoenix_amd import _lib
    return _lib.load().phx_debug_calls_grids_kernel_m(N, H, B * K, T, K, _lib.METHODS[method])


@pytest.mark.parametrize("N,H,B,K,method,tdtype", [
    (350, 30, 7, 6, "dopri5", np.float64), (350, 30, 60, 4, "dopri5", np.float32), (11165, 40, 60, 3, "dopri5", np.float64),
    (96, 8, 5, 40, "dopri5", np.float64), (14691, 200, 24, 2, "dopri5", np.float64), (700, 20, 20, 3, "rk4", np.float64)])
def test_calls_with_their_own_grids_equal_separate_calls(pa, dev, oracle, N, H, B, K, method, tdtype):
    p = rand_params(N, H, seed=N + K, std=0.6 / np.sqrt(N))
    net = make_net(pa, dev, p)
    T = 6
    y0s, tg = _y0s(N, B, K), _grids(K, T, tdtype)
    y0d, td = torch.from_numpy(y0s).to(dev), torch.from_numpy(tg).to(dev)
    kern = _kernel(N, H, B, T, K, method)
    assert kern == (1 if method != "dopri5" else (3 if H <= 48 else 4))      # dopri5: the third-generation kernels
    out = pa.odeint_calls(net, y0d, td, method=method)
    assert out.shape == (K, T, B, 1, N)
    tol = TOL_DOPRI if method == "dopri5" else TOL_FIXED_CALLS
    steps = []
    for k in range(K):
        one, _nfe, nsteps = pa.odeint(net, y0d[k], td[k], method=method, return_stats=True)
        steps.append(int(nsteps[0]))
        e = relerr(out[k].cpu().numpy(), one.cpu().numpy())
        print("call", k, "relerr", e, "nsteps", steps[-1])
        assert e < tol, k
    if method == "dopri5" and N <= 700:
        assert len(set(steps)) > 1
    if N <= 2000:
        k = K - 1
        ref = oracle.odeint(onet_of(oracle, p), y0s[k], tg[k].astype(np.float64), method=method)
        e = relerr(out[k].cpu().numpy(), ref)
        print("oracle relerr", e)
        assert e < TOL_DOPRI
    with pytest.raises(ValueError):
        pa.odeint_calls(net, y0d, td[:-1] if K > 2 else torch.cat([td, td]), method=method)


def _solve(pa, dev, p, y0s, tg, method="dopri5"):
    """engine.solve_forward on K calls with their grids -> sol [T, K, B, N], status / nsteps [K, B]"""
    from phoenix_amd import _lib, engine
    K, B, _, N = y0s.shape
    net = make_net(pa, dev, p)
    prm = engine.params_cached(*pa.odenet.params_of(net))
    y2 = torch.from_numpy(y0s.reshape(K * B, N)).to(dev)
    sol, status, _nfe, nsteps = engine.solve_forward(prm, y2, torch.from_numpy(tg).to(dev), method, _lib.CTRL_SHARED, 1e-7,
                                                     1e-9, True, 0, calls=K)
    torch.cuda.synchronize()
    engine.forget_workspaces()
    return (sol.reshape(tg.shape[1], K, B, N).cpu().numpy(), status.reshape(K, B).cpu().numpy(),
            nsteps.reshape(K, B).cpu().numpy())


def test_every_call_has_its_own_controller(pa, dev):
    N, H, B, K = 350, 30, 20, 5
    p = rand_params(N, H, seed=11, std=0.6 / np.sqrt(N))
    _sol, status, nsteps = _solve(pa, dev, p, _y0s(N, B, K), _grids(K, 5, np.float64))
    assert (status == 0).all()
    assert (nsteps == nsteps[:, :1]).all()             # one controller for the rows of a call
    assert len(set(nsteps[:, 0].tolist())) > 1         # ... and not the same one for every call


def test_a_failing_call_leaves_its_neighbours_alone(pa, dev):
    N, H, B, K = 350, 30, 20, 4
    p = rand_params(N, H, seed=12, std=0.6 / np.sqrt(N))
    y0s, tg = _y0s(N, B, K), _grids(K, 5, np.float64)
    good, st0, _ = _solve(pa, dev, p, y0s, tg)
    assert (st0 == 0).all()
    bad = y0s.copy()
    bad[2] = np.nan
    sol, status, _ = _solve(pa, dev, p, bad, tg)
    assert (status[2] != 0).all() and np.isnan(sol[1:, 2]).all()
    for k in (0, 1, 3):
        assert (status[k] == 0).all() and np.isfinite(sol[:, k]).all()
        assert np.array_equal(sol[:, k], good[:, k])
    net = make_net(pa, dev, p)
    with pytest.raises(AssertionError):
        pa.odeint_calls(net, torch.from_numpy(bad).to(dev), torch.from_numpy(tg).to(dev), method="dopri5")
    pa.engine.forget_workspaces()


def test_more_calls_than_one_launch_takes(pa, dev):
    from phoenix_amd import _lib
    N, H, B, T = 96, 8, 5, 4
    lib = _lib.load()
    plan = (C.c_int * 6)()
    K = 300
    n = lib.phx_debug_calls_grids_plan(N, H, B * K, T, K, _lib.METHODS["dopri5"], plan)
    assert 1 <= n < K and plan[0] == 3 and plan[1] * plan[2] <= plan[5] == lib.phx_device_cus()
    assert lib.phx_debug_calls_grids_launches(N, H, B * K, T, K, _lib.METHODS["dopri5"]) == -(-K // n) > 1
    p = rand_params(N, H, seed=13, std=0.6 / np.sqrt(N))
    net = make_net(pa, dev, p)
    rs = np.random.RandomState(3)
    y0s = (rs.rand(K, B, 1, N).astype(np.float32) - 0.5) * (0.2 + rs.rand(K, 1, 1, 1).astype(np.float32) * 3)
    tg = np.stack([_grids(3, T, np.float64)[k % 3] + 0.01 * k for k in range(K)])
    y0d, td = torch.from_numpy(y0s).to(dev), torch.from_numpy(tg).to(dev)
    out = pa.odeint_calls(net, y0d, td, method="dopri5")
    for k in (0, 1, n - 1, n, n + 1, K - 1):
        with torch.no_grad():
            one = pa.odeint(net, y0d[k], td[k], method="dopri5")
        assert relerr(out[k].cpu().numpy(), one.cpu().numpy()) < TOL_DOPRI, k


def test_valu_engine_falls_back_to_separate_calls(pa, dev, monkeypatch):
    N, H, B, K, T = 96, 8, 5, 4, 4
    p = rand_params(N, H, seed=14, std=0.6 / np.sqrt(N))
    net = make_net(pa, dev, p)
    y0d = torch.from_numpy(_y0s(N, B, K)).to(dev)
    td = torch.from_numpy(_grids(K, T, np.float64)).to(dev)
    ref = pa.odeint_calls(net, y0d, td, method="dopri5").cpu().numpy()
    monkeypatch.setenv("PHX_ENGINE", "v0")
    pa.engine.forget_workspaces()
    assert _kernel(N, H, B, T, K, "dopri5") == 0
    got = pa.odeint_calls(net, y0d, td, method="dopri5").cpu().numpy()
    monkeypatch.delenv("PHX_ENGINE")
    pa.engine.forget_workspaces()
    assert relerr(got, ref) < TOL_FIXED_CALLS
