"""CPU-only checks of the combination knockout screen's boundaries (phx_odeint_clamped_sets, phx_knockout_epistasis and
its size query, include/phoenix_hip.h; `odeint_calls(clamp=<sets>)`, `knockout_pairs`): the symbols exist, every argument
check answers before a device call -- and `reference64_pairs`, the float64 restatement of the scoring formulas that
tests/test_knockout_pairs_gpu.py holds the kernel to."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

from test_abi_cpu import _declared_symbols

BAD_ARG, WORKSPACE = 4, 5
NEW = ("phx_odeint_clamped_sets", "phx_knockout_epistasis_workspace_bytes", "phx_knockout_epistasis")


def _lib():
    from phoenix_amd import _lib
    return _lib, _lib.load()


def reference64_pairs(base, singles, sol, ia, ib, genes):
    """the formulas of include/phoenix_hip.h (phx_knockout_epistasis) in float64 numpy: base [T, B, N], singles
    [T, G*B, N], sol [T, K*B, N], pair k = singles (ia[k], ib[k]), genes[g] the held gene of single g ->
    (scores [K], interaction_scores [K], shift, magnitude, interaction, interaction_magnitude [K, N]).
    The arbiter of the GPU tests."""
    base, singles, sol = (np.asarray(x, np.float64) for x in (base, singles, sol))
    T, B, N = base.shape
    K, G = len(ia), len(genes)
    assert len(ib) == K and singles.shape == (T, G * B, N) and sol.shape == (T, K * B, N)
    d1 = singles[1:].reshape(T - 1, G, B, N) - base[1:, None]
    dab = sol[1:].reshape(T - 1, K, B, N) - base[1:, None]
    e = dab - (d1[:, list(ia)] + d1[:, list(ib)])
    shift, magnitude = dab.mean(axis=(0, 2)), np.abs(dab).mean(axis=(0, 2))
    interaction, interaction_magnitude = e.mean(axis=(0, 2)), np.abs(e).mean(axis=(0, 2))
    scores, iscores = np.empty(K), np.empty(K)
    for k in range(K):
        keep = np.ones(N, bool)
        keep[[genes[ia[k]], genes[ib[k]]]] = False
        scores[k] = magnitude[k, keep].mean()
        iscores[k] = interaction_magnitude[k, keep].mean()
    return scores, iscores, shift, magnitude, interaction, interaction_magnitude


def test_reference64_pairs_on_a_case_worked_by_hand():
    # T = 2, B = 1, N = 4: one output row per solve.  Singles hold genes 3 and 1, the pair holds both.
    base = np.array([[[9.0, 9.0, 9.0, 9.0]], [[1.0, 2.0, 3.0, 4.0]]])
    singles = np.zeros((2, 2, 4))
    singles[0] = 77.0                                # the initial states are not part of any mean
    singles[1, 0] = [2.0, 2.5, 3.0, 0.0]             # single 0 (gene 3): d_a = [1, 0.5, 0, -4]
    singles[1, 1] = [0.0, 0.0, 5.0, 4.5]             # single 1 (gene 1): d_b = [-1, -2, 2, 0.5]
    sol = np.zeros((2, 1, 4))
    sol[0] = -55.0
    sol[1, 0] = [3.0, 0.0, 2.0, 0.0]                 # the pair: d_ab = [2, -2, -1, -4];  e = d_ab - (d_a + d_b) = [2, -0.5, -3, -0.5]
    sc, isc, sh, mg, it, im = reference64_pairs(base, singles, sol, [0], [1], [3, 1])
    assert np.allclose(sh, [[2, -2, -1, -4]]) and np.allclose(mg, [[2, 2, 1, 4]])
    assert np.allclose(it, [[2, -0.5, -3, -0.5]]) and np.allclose(im, [[2, 0.5, 3, 0.5]])
    assert np.allclose(sc, [(2 + 1) / 2]) and np.allclose(isc, [(2 + 3) / 2])      # columns 1 and 3 are left out
    # the other order of the pair: the same numbers
    for x, y in zip(reference64_pairs(base, singles, sol, [1], [0], [3, 1]), (sc, isc, sh, mg, it, im)):
        assert np.array_equal(x, y)


def test_new_symbols_are_exported_and_declared():
    mod, lib = _lib()
    for name in NEW:
        assert name in mod.EXPORTS and name in _declared_symbols() and hasattr(lib, name), name
    assert lib.phx_abi_version() == 7       # an additive change
    from phoenix_amd import engine
    src = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "phoenix_hip.h")).read()
    assert "#define PHX_CLAMP_MAX %d" % engine.CLAMP_MAX in src


# --------------------------------------------------------------------------- phx_odeint_clamped_sets
def _solve(lib, mod, N=96, H=8, B=30, T=5, calls=6, method="dopri5", control=None, per_sample=1, clamp=0x5000, width=2,
           y0=0x1000, t=0x2000, sol=0x3000, ws=0x4000, opts=True):
    """phx_odeint_clamped_sets with made-up device addresses: only calls that must return before touching the device"""
    x = C.cast((C.c_float * 4)(), C.c_void_p)
    prm = mod.PhxParams(x, x, x, x, x, x, N, H, None)
    o = mod.PhxSolveOpts(mod.METHODS[method], mod.CTRL_SHARED if control is None else control, 1e-7, 1e-9, per_sample, 0, 0,
                         calls, 0)
    return lib.phx_odeint_clamped_sets(C.byref(prm), y0, t, B, T, C.byref(o) if opts else None, clamp, width, sol, 0x6000,
                                       0x6100, 0x6200, ws, 1 << 30, None)


def test_clamped_sets_solve_rejects_bad_arguments_before_any_device_call(monkeypatch):
    mod, lib = _lib()
    for width in (0, -1, 5, 1 << 20):
        assert _solve(lib, mod, width=width) == BAD_ARG, width
    for width in (1, 2, 3, 4):
        assert _solve(lib, mod, width=width, clamp=None) == BAD_ARG, width
    # everything phx_odeint_clamped refuses
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


# --------------------------------------------------------------------------- phx_knockout_epistasis
def _score(lib, base=0x1000, singles=0x1800, sol=0x2000, T=10, K=2, G=3, B=3, N=8, ia=(0, 1), ib=(1, 2), genes=(0, 7, 3),
           scores=0x3000, iscores=0x3100, mats=(None, None, None, None), ws=0x4000, ws_bytes=None):
    if ws_bytes is None:
        ws_bytes = max(lib.phx_knockout_epistasis_workspace_bytes(T, K, G, B, N), 1 << 20)
    arr = lambda v: None if v is None else (C.c_int * len(v))(*v)      # noqa: E731
    return lib.phx_knockout_epistasis(base, singles, sol, T, K, G, B, N, arr(ia), arr(ib), arr(genes), scores, iscores,
                                      mats[0], mats[1], mats[2], mats[3], ws, ws_bytes, None)


def test_epistasis_rejects_bad_arguments_before_any_device_call():
    _, lib = _lib()
    for kw in (dict(base=None), dict(singles=None), dict(sol=None), dict(ia=None), dict(ib=None), dict(genes=None),
               dict(scores=None), dict(iscores=None), dict(T=1), dict(K=0), dict(K=65536, ia=(0,) * 65536, ib=(1,) * 65536),
               dict(G=1), dict(G=0), dict(B=0), dict(N=2, genes=(0, 1, 0)), dict(N=-1),
               dict(ia=(0, 3)),            # G = 3: the last single is 2
               dict(ib=(1, -1)),
               dict(ia=(0, 2), ib=(1, 2)),      # a pair of a single with itself
               dict(genes=(0, 8, 3)),      # N = 8: the last gene is 7
               dict(genes=(0, 7, -1))):
        assert _score(lib, **kw) == BAD_ARG, kw
    need = lib.phx_knockout_epistasis_workspace_bytes(10, 2, 3, 3, 8)
    assert need >= 2 * 2 * 8 * 4
    assert _score(lib, ws_bytes=need - 1) == WORKSPACE
    assert _score(lib, ws_bytes=need - 1, mats=(0x5000, 0x5100, 0x5200, 0x5300)) == WORKSPACE
    assert _score(lib, ws=None) == WORKSPACE
    assert _score(lib, T=1, ws_bytes=0) == BAD_ARG      # the argument checks come first
    f = lib.phx_knockout_epistasis_workspace_bytes
    for shape in ((1, 8, 4, 60, 350), (10, 0, 4, 60, 350), (10, 8, 1, 60, 350), (10, 8, 4, 0, 350), (10, 8, 4, 60, 2),
                  (-1, 8, 4, 60, 350), (10, 65536, 4, 60, 350)):
        assert f(*shape) == 0, shape
    sizes = [f(10, k, 4, 60, 350) for k in (1, 2, 8, 40)]
    assert sizes[0] > 0 and sizes == sorted(sizes)


# --------------------------------------------------------------------------- odeint_calls(clamp=<sets>)
def _net(N=16, H=4):
    import phoenix_amd
    return phoenix_amd.ODENet("cpu", N, neurons=H)


def test_clamp_list_takes_nested_lists_and_the_2d_tensor():
    from phoenix_amd.odeint import _clamp_list
    assert _clamp_list([3, [1, 2], (), -1, [5, 5, 4], (7, -1), np.array([9, 8])], 7, 16) == \
        [(3,), (1, 2), (), (), (4, 5), (7,), (8, 9)]
    assert _clamp_list([[0, 1, 2, 15]], 1, 16) == [(0, 1, 2, 15)]
    t2 = torch.tensor([[0, 15, -1, -1], [-1, -1, -1, -1], [3, 3, 2, 1]], dtype=torch.int32)
    assert _clamp_list(t2, 3, 16) == [(0, 15), (), (1, 2, 3)]
    assert _clamp_list(t2.long()[:, :1], 3, 16) == [(0,), (), (3,)]
    assert _clamp_list(torch.tensor([0, -1, 15]), 3, 16) == [(0,), (), (15,)]      # as before
    assert _clamp_list(np.array([[0, 1], [2, -1]]), 2, 16) == [(0, 1), (2,)]


@pytest.mark.parametrize("clamp,exc", [([0, [1, 2, 3, 4, 5], 2], ValueError),        # a set of 5
                                       ([0, [1, -1, -1, -1, -1], 2], ValueError),    # ... padding included
                                       (torch.zeros((3, 5), dtype=torch.int64), ValueError),
                                       ([0, [1, 2.0], 2], TypeError),                # a float entry
                                       ([0, [1, True], 2], TypeError),
                                       (torch.zeros((3, 2)), TypeError),
                                       (torch.zeros((3, 2, 1), dtype=torch.int32), TypeError),
                                       ([0, [1, 16], 2], ValueError),                # N = 16: the last gene is 15
                                       ([0, [1, -2], 2], ValueError),
                                       ([[0, 1], [2, 3]], ValueError),               # two sets for three calls
                                       (torch.zeros((2, 2), dtype=torch.int32), ValueError)])
def test_odeint_calls_checks_the_clamp_sets_on_the_host(clamp, exc):
    import phoenix_amd
    y0s, t = torch.zeros(3, 2, 1, 16), torch.linspace(0, 1, 4, dtype=torch.float64)
    with pytest.raises(exc, match="clamp"):
        phoenix_amd.odeint_calls(_net(), y0s, t, clamp=clamp)


def test_good_clamp_sets_reach_the_device_requirement():
    import phoenix_amd
    y0s, t = torch.zeros(3, 2, 1, 16), torch.linspace(0, 1, 4, dtype=torch.float64)
    for clamp in ([0, [1, 2], ()], torch.tensor([[0, 1], [2, -1], [-1, -1]]), [[0, 1, 2, 3], [4], -1]):
        with pytest.raises(RuntimeError, match="no CPU path|must live on the GPU"):
            phoenix_amd.odeint_calls(_net(), y0s, t, clamp=clamp)


# --------------------------------------------------------------------------- knockout_pairs
@pytest.mark.parametrize("kw,exc", [(dict(), ValueError),                                        # neither genes nor pairs
                                    (dict(pairs=[(0, 1), (2, 2)]), ValueError),                  # a pair (a, a)
                                    (dict(pairs=[(0, 1), (2, 3), (1, 0)]), ValueError),          # a pair twice, the other order
                                    (dict(pairs=[(0, 1), (0, 1)]), ValueError),
                                    (dict(genes=[0, 1, 2], value=[0.0, 1.0]), ValueError),       # two levels for three genes
                                    (dict(pairs=[(0, 5), (5, 9)], value=[0.0, 1.0]), ValueError),   # ... three genes again
                                    (dict(genes=[0, 1], max_singles_bytes=4 * 10 * 2 * 2 * 16 - 1), ValueError),
                                    (dict(genes=[0]), ValueError), (dict(genes=[0, 0]), ValueError),
                                    (dict(genes=[0, 16]), ValueError), (dict(pairs=[(0, 16)]), ValueError),
                                    (dict(pairs=[]), ValueError), (dict(pairs=[(0, 1, 2)]), ValueError),
                                    (dict(genes=[0, 1], pairs=[(0, 2)]), ValueError),
                                    (dict(genes=[0, 1.5]), TypeError), (dict(pairs=[(0, 1.5)]), TypeError),
                                    (dict(genes=[0, 1], pairs_per_launch=0), ValueError)])
def test_knockout_pairs_checks_its_arguments_before_a_device_is_needed(kw, exc):
    import phoenix_amd
    with pytest.raises(exc, match="knockout_pairs"):
        phoenix_amd.knockout_pairs(_net(), torch.zeros(2, 1, 16), **kw)


def test_the_singles_size_guard_names_the_size():
    import phoenix_amd
    nbytes = 4 * 10 * 3 * 2 * 16      # 4 T G B N with the default grid of 10 points
    with pytest.raises(ValueError, match=str(nbytes)):
        phoenix_amd.knockout_pairs(_net(), torch.zeros(2, 1, 16), genes=[0, 1, 2], max_singles_bytes=nbytes - 1)
    with pytest.raises(RuntimeError, match="no CPU path|must live on the GPU"):      # at the limit: the next thing is the GPU
        phoenix_amd.knockout_pairs(_net(), torch.zeros(2, 1, 16), genes=[0, 1, 2], max_singles_bytes=nbytes)


def test_knockout_pairs_has_no_cpu_path():
    import phoenix_amd
    with pytest.raises(ValueError, match="y0 must be"):
        phoenix_amd.knockout_pairs(_net(), torch.zeros(2, 1, 15), genes=[0, 1])
    with pytest.raises(RuntimeError, match="no CPU path|must live on the GPU"):
        phoenix_amd.knockout_pairs(_net(), torch.zeros(2, 1, 16), pairs=[(0, 3), (3, 5)])
    from phoenix_amd import engine
    with pytest.raises(RuntimeError, match="no CPU path|must live on the GPU"):
        engine.knockout_epistasis(torch.zeros(4, 2, 16), torch.zeros(4, 4, 16), torch.zeros(4, 2, 16), [0], [1], [0, 3])


def test_pairs_and_genes_of_a_screen():
    from phoenix_amd.analysis import _knockout_pairs_args
    genes, values, pairs, ia, ib = _knockout_pairs_args(16, [5, 2, 9], None, [1.0, 2.0, 3.0], 8)
    assert genes == [5, 2, 9] and values == [1.0, 2.0, 3.0] and pairs == [(5, 2), (5, 9), (2, 9)]
    assert ia == [0, 0, 1] and ib == [1, 2, 2]
    genes, values, pairs, ia, ib = _knockout_pairs_args(16, None, [(9, 2), (2, 5)], 2.0, 1)
    assert genes == [2, 5, 9] and values == [2.0] * 3 and pairs == [(9, 2), (2, 5)] and ia == [2, 0] and ib == [0, 1]
