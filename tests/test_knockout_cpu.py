"""CPU-only checks of the knockout screen's boundaries (phx_odeint_clamped, phx_knockout_effects and their size queries,
include/phoenix_hip.h; `odeint_calls(clamp=...)`, `knockout_effects`): the symbols exist, the clamped plan exists exactly
where dopri5 runs on the third-generation kernels, every argument check answers before a device call -- and the float64
restatement of the scoring formulas that tests/test_knockout_gpu.py holds the kernel to."""
import ctypes as C

import numpy as np
import pytest
import torch

from test_abi_cpu import _declared_symbols

BAD_ARG, WORKSPACE = 4, 5
NEW = ("phx_odeint_clamped_workspace_bytes", "phx_odeint_clamped", "phx_knockout_effects_workspace_bytes",
       "phx_knockout_effects")


def _lib():
    from phoenix_amd import _lib
    return _lib, _lib.load()


def reference64(base, sol, genes):
    """the formulas of include/phoenix_hip.h (phx_knockout_effects) in float64 numpy: base [T, B, N], sol [T, K*B, N] ->
    (scores [K], shift [K, N], magnitude [K, N]).  The arbiter of the GPU tests."""
    base, sol = np.asarray(base, np.float64), np.asarray(sol, np.float64)
    T, B, N = base.shape
    K = len(genes)
    assert sol.shape == (T, K * B, N)
    d = sol[1:].reshape(T - 1, K, B, N) - base[1:, None]
    shift = d.mean(axis=(0, 2))
    magnitude = np.abs(d).mean(axis=(0, 2))
    scores = np.empty(K)
    for k in range(K):
        keep = np.ones(N, bool)
        keep[genes[k]] = False
        scores[k] = magnitude[k, keep].mean()
    return scores, shift, magnitude


def test_reference64_on_a_case_worked_by_hand():
    base = np.zeros((3, 2, 3))
    sol = np.zeros((3, 4, 3))
    sol[0] = 99.0                        # the initial states are not part of any mean
    sol[1:, 0:2, 1] = [[1.0, -3.0], [2.0, 2.0]]      # knockout 0, target 1: d = 1, -3, 2, 2
    sol[1:, 2:4, 0] = 5.0                # knockout 1 clamps gene 0 itself: left out of its score
    sol[1:, 2:4, 2] = -0.5
    scores, shift, magnitude = reference64(base, sol, [0, 0])
    assert np.allclose(shift[0], [0, 0.5, 0]) and np.allclose(magnitude[0], [0, 2.0, 0])
    assert np.allclose(shift[1], [5.0, 0, -0.5]) and np.allclose(magnitude[1], [5.0, 0, 0.5])
    assert np.allclose(scores, [1.0, 0.25])


def test_new_symbols_are_exported_and_declared():
    mod, lib = _lib()
    for name in NEW:
        assert name in mod.EXPORTS and name in _declared_symbols() and hasattr(lib, name), name
    assert lib.phx_abi_version() == 7       # an additive change


@pytest.mark.parametrize("N,H,B,K", [(96, 8, 5, 6), (96, 44, 5, 4), (96, 56, 5, 4), (350, 200, 7, 3), (350, 30, 7, 1),
                                     (350, 30, 300, 2),       # 300 rows per call: only the first-generation kernel plans them
                                     (350, 300, 7, 3)])       # H > 256: the same
def test_clamped_plan_exists_where_dopri5_runs_on_the_third_generation(N, H, B, K):
    mod, lib = _lib()
    T = 5
    for method, name in ((3, "dopri5"), (2, "rk4")):
        assert mod.METHODS[name] == method
    kern = lib.phx_debug_calls_grids_kernel_m(N, H, B * K, T, K, mod.METHODS["dopri5"])
    nbytes = lib.phx_odeint_clamped_workspace_bytes(N, H, B * K, T, K)
    print("N=%d H=%d B=%d K=%d: kernel %d, %d bytes" % (N, H, B, K, kern, nbytes))
    assert (nbytes > 0) == (kern in (3, 4))
    assert kern == (1 if (B > 256 or H > 256) else (3 if H <= 48 else 4))
    if nbytes:      # the planning of the calls with their own grids, nothing new
        assert nbytes == lib.phx_odeint_calls_grids_workspace_bytes(N, H, B * K, T, K, mod.METHODS["dopri5"]) or K == 1
    assert lib.phx_odeint_clamped_workspace_bytes(N, H, B * K + 1, T, K) == 0 or K == 1      # not K equal calls
    assert lib.phx_odeint_clamped_workspace_bytes(N, H, B * K, T, 0) == 0


def test_clamped_plan_is_gone_with_the_valu_engine(monkeypatch):
    _, lib = _lib()
    assert lib.phx_odeint_clamped_workspace_bytes(96, 8, 30, 5, 6) > 0
    monkeypatch.setenv("PHX_ENGINE", "v0")
    assert lib.phx_odeint_clamped_workspace_bytes(96, 8, 30, 5, 6) == 0


def _solve(lib, mod, N=96, H=8, B=30, T=5, calls=6, method="dopri5", control=None, per_sample=1, clamp=0x5000, y0=0x1000,
           t=0x2000, sol=0x3000, ws=0x4000, opts=True):
    """phx_odeint_clamped with made-up device addresses: only calls that must return before touching the device"""
    x = C.cast((C.c_float * 4)(), C.c_void_p)
    prm = mod.PhxParams(x, x, x, x, x, x, N, H, None)
    o = mod.PhxSolveOpts(mod.METHODS[method], mod.CTRL_SHARED if control is None else control, 1e-7, 1e-9, per_sample, 0, 0,
                         calls, 0)
    return lib.phx_odeint_clamped(C.byref(prm), y0, t, B, T, C.byref(o) if opts else None, clamp, sol, 0x6000, 0x6100, 0x6200,
                                  ws, 1 << 30, None)


def test_clamped_solve_rejects_bad_arguments_before_any_device_call(monkeypatch):
    mod, lib = _lib()
    assert _solve(lib, mod, clamp=None) == BAD_ARG
    for m in ("euler", "midpoint", "rk4"):
        assert _solve(lib, mod, method=m) == BAD_ARG
    assert _solve(lib, mod, control=mod.CTRL_PER_TRAJECTORY) == BAD_ARG
    assert _solve(lib, mod, per_sample=0) == BAD_ARG
    assert _solve(lib, mod, B=31) == BAD_ARG              # B % calls
    assert _solve(lib, mod, calls=0) == BAD_ARG
    assert _solve(lib, mod, y0=None) == BAD_ARG and _solve(lib, mod, t=None) == BAD_ARG
    assert _solve(lib, mod, sol=None) == BAD_ARG and _solve(lib, mod, ws=None) == BAD_ARG
    assert _solve(lib, mod, opts=False) == BAD_ARG
    assert _solve(lib, mod, N=350, H=30, B=600, calls=2) == BAD_ARG      # the first-generation kernel's shape: no clamp
    monkeypatch.setenv("PHX_ENGINE", "v0")
    assert _solve(lib, mod) == BAD_ARG                    # no third-generation kernel at all


def _score(lib, base=0x1000, sol=0x2000, T=10, K=2, B=3, N=8, genes=(0, 7), scores=0x3000, shift=None, magnitude=None,
           ws=0x4000, ws_bytes=None):
    if ws_bytes is None:
        ws_bytes = max(lib.phx_knockout_effects_workspace_bytes(T, K, B, N), 1 << 20)
    g = None if genes is None else (C.c_int * len(genes))(*genes)
    return lib.phx_knockout_effects(base, sol, T, K, B, N, g, scores, shift, magnitude, ws, ws_bytes, None)


def test_scoring_rejects_bad_arguments_before_any_device_call():
    _, lib = _lib()
    assert _score(lib, base=None) == BAD_ARG
    assert _score(lib, sol=None) == BAD_ARG
    assert _score(lib, scores=None) == BAD_ARG
    assert _score(lib, genes=None) == BAD_ARG
    assert _score(lib, T=1) == BAD_ARG
    assert _score(lib, K=0, genes=(0,)) == BAD_ARG
    assert _score(lib, K=65536, genes=(0,) * 65536) == BAD_ARG
    assert _score(lib, B=0) == BAD_ARG
    assert _score(lib, N=1, genes=(0, 0)) == BAD_ARG
    assert _score(lib, genes=(0, 8)) == BAD_ARG        # N = 8: the last valid index is 7
    assert _score(lib, genes=(-1, 3)) == BAD_ARG
    need = lib.phx_knockout_effects_workspace_bytes(10, 2, 3, 8)
    assert need >= 2 * 8 * 4
    assert _score(lib, ws_bytes=need - 1) == WORKSPACE
    assert _score(lib, ws_bytes=need - 1, shift=0x5000, magnitude=0x6000) == WORKSPACE
    assert _score(lib, ws=None) == WORKSPACE
    assert _score(lib, T=1, ws_bytes=0) == BAD_ARG      # the argument checks come first
    f = lib.phx_knockout_effects_workspace_bytes
    for shape in ((1, 8, 60, 350), (10, 0, 60, 350), (10, 8, 0, 350), (10, 8, 60, 1), (-1, 8, 60, 350), (10, 65536, 60, 350)):
        assert f(*shape) == 0, shape
    sizes = [f(10, k, 60, 350) for k in (1, 2, 8, 40)]
    assert sizes[0] > 0 and sizes == sorted(sizes)


def _net(N=16, H=4):
    import phoenix_amd
    return phoenix_amd.ODENet("cpu", N, neurons=H)


@pytest.mark.parametrize("clamp,exc", [([0, 1], ValueError),            # two genes for three calls
                                       ([0, 1, 16], ValueError),        # N = 16: the last gene is 15
                                       ([0, -2, 1], ValueError),        # -1 alone means none
                                       ([0, 1.5, 2], TypeError), (torch.tensor([0.0, 1.0, 2.0]), TypeError),
                                       ([0, True, 2], TypeError), (7, TypeError)])
def test_odeint_calls_checks_the_clamp_list_on_the_host(clamp, exc):
    import phoenix_amd
    y0s, t = torch.zeros(3, 2, 1, 16), torch.linspace(0, 1, 4, dtype=torch.float64)
    with pytest.raises(exc, match="clamp"):
        phoenix_amd.odeint_calls(_net(), y0s, t, clamp=clamp)


def test_a_good_clamp_list_reaches_the_device_requirement():
    """numpy and tensor integers pass the host checks; the next thing asked for is the GPU"""
    import phoenix_amd
    y0s, t = torch.zeros(3, 2, 1, 16), torch.linspace(0, 1, 4, dtype=torch.float64)
    for clamp in ([0, -1, 15], np.array([0, -1, 15]), torch.tensor([0, -1, 15], dtype=torch.int32)):
        with pytest.raises(RuntimeError, match="no CPU path|must live on the GPU"):
            phoenix_amd.odeint_calls(_net(), y0s, t, clamp=clamp)


@pytest.mark.parametrize("kw,exc", [(dict(genes=[0, 16]), ValueError), (dict(genes=[-1]), ValueError),
                                    (dict(genes=[0.5]), TypeError), (dict(genes=[]), ValueError),
                                    (dict(genes=[0, 1], value=[0.0]), ValueError),          # one level for two genes
                                    (dict(genes=[0, 1], genes_per_launch=0), ValueError)])
def test_knockout_effects_checks_its_arguments_on_the_host(kw, exc):
    import phoenix_amd
    with pytest.raises(exc, match="knockout_effects"):
        phoenix_amd.knockout_effects(_net(), torch.zeros(2, 1, 16), **kw)


def test_knockout_effects_has_no_cpu_path():
    import phoenix_amd
    with pytest.raises(ValueError, match="y0 must be"):
        phoenix_amd.knockout_effects(_net(), torch.zeros(2, 1, 15), genes=[0])
    with pytest.raises(RuntimeError, match="no CPU path|must live on the GPU"):
        phoenix_amd.knockout_effects(_net(), torch.zeros(2, 1, 16), genes=[0, 3])
    from phoenix_amd import engine
    with pytest.raises(RuntimeError, match="no CPU path|must live on the GPU"):
        engine.knockout_effects(torch.zeros(4, 2, 16), torch.zeros(4, 4, 16), [0, 3])
