"""k3_tail_adj3 (phx_mfma_adj3_tail.inc): a batch group of k1_solve_adj3 whose trajectories all end the backward solve in
its first accepted step leaves that step's quadrature + accept pass to the launch behind the solve, which also sums the
groups and writes the caller's gradients.  Every case is solved with the tail kernel on (the default from four trajectory
tiles per launch on, `PHX_V3_TAIL=1` below) and off (`PHX_V3_TAIL=0`: the solve runs every visit, k3_reduce_grads sums) and both are held to the CPU oracle at the dopri5 gradient bar of
tests/test_gpu_parity.py; the workspace's words (phx_debug_adj3_tail_words) say which groups deferred and that the tail
launch served them.  Shapes: N = 200 is seven gene blocks, the last with 8 genes (B = 5: the waves split the blocks, 11
padding trajectories); N = 1100, H = 48 has a full last hidden tile (B = 19: two tiles, 13 padding trajectories); N = 1100,
H = 33, B = 80 plans more than one batch group (asserted).  On the MI355X; run with `-m gpu`."""
import ctypes as C

import numpy as np
import pytest
import torch

from conftest import grad_err
from test_gpu_parity import KEYS, TOL_DOPRI_GRAD, make_net, onet_of, rand_params

pytestmark = pytest.mark.gpu

SHAPES = [(200, 40, 5), (1100, 48, 19), (1100, 33, 80)]
T_END = 0.005     # one accepted step (asserted)
T_LONG = 1.0      # several steps
_problems = {}


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "these tests need the MI355X"
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def pa():
    import phoenix_amd
    return phoenix_amd


@pytest.fixture(autouse=True)
def third_backward_kernel(monkeypatch):
    """the planner gives these small shapes to k1_solve_adj2: PHX_ADJ=v3 puts them on k1_solve_adj3 (asserted in solve)"""
    monkeypatch.setenv("PHX_ADJ", "v3")


def plan_of(N, H, B, T):
    """(TG, Bt) of k1_solve_adj3's launch for this batch on this device"""
    from phoenix_amd import _lib
    lib = _lib.load()
    out = (C.c_longlong * 37)()
    assert lib.phx_debug_plan(_lib.OP_ADJOINT, 3, lib.phx_device_cus(), N, H, B, T, _lib.CTRL_PER_TRAJECTORY,
                              _lib.METHODS["dopri5"], 1, out)
    return int(out[9]), int(out[12])


def same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and bool(((a.view(np.uint32) == b.view(np.uint32)) | ((a == 0) & (b == 0))).all())


def problem(oracle, N, H, B, grid):
    """parameters (a tenth of the gene multipliers negative), states, per-sample time rows, cotangents and the oracle's
    adjoint results of them; computed once per (shape, grid)"""
    key = (N, H, B, grid)
    if key in _problems:
        return _problems[key]
    p = rand_params(N, H, seed=3 * N + H, std=0.05)
    r = np.random.RandomState(17 + B)
    y0 = np.clip(r.randn(B, N) * 0.15 + 0.5, 0.03, 1.07).astype(np.float32)
    if grid == "one":
        t = np.tile(np.array([0.0, T_END], np.float32), (B, 1))
    elif grid == "mixed":                  # the rows of the LAST batch group integrate over [0, 1]
        _, Bt = plan_of(N, H, B, 2)
        t = np.tile(np.array([0.0, T_END], np.float32), (B, 1))
        t[(B - 1) // Bt * Bt:, 1] = T_LONG
    else:                                  # three time points
        t = np.tile(np.array([0.0, 0.5 * T_END, T_END], np.float32), (B, 1))
    G = r.randn(B, t.shape[1], N).astype(np.float32)
    onet = onet_of(oracle, p)
    ref = oracle.odeint_per_sample(onet, y0, t, method="dopri5")
    adj_ref, gr_ref = oracle.adjoint_backward_per_sample(onet, t, ref, G, method="dopri5", theta_in_norm=True)
    _problems[key] = (p, y0, t, G, adj_ref, gr_ref)
    return _problems[key]


def solve(pa, dev, monkeypatch, p, y0, t, G, tail, want_grads=True):
    """forward + backward solve through the engine with the tail kernel on / off -> adj_y0, gradients (dict or None),
    nsteps of the backward solve, the groups' deferred words and the served word of the workspace"""
    from phoenix_amd import _lib, engine
    N, H, B, T = y0.shape[1], p["Ws"].shape[0], y0.shape[0], t.shape[1]
    if tail and B > 48:       # at least four trajectory tiles: the tail kernel is the default
        monkeypatch.delenv("PHX_V3_TAIL", raising=False)
    elif tail:                # smaller launches keep the in-kernel visit unless told otherwise
        monkeypatch.setenv("PHX_V3_TAIL", "1")
    else:
        monkeypatch.setenv("PHX_V3_TAIL", "0")
    lib = _lib.load()
    assert lib.phx_debug_adjoint_kernel_m(N, H, B, T, _lib.CTRL_PER_TRAJECTORY, _lib.METHODS["dopri5"]) == 3
    off_d, off_s = C.c_size_t(0), C.c_size_t(0)
    assert lib.phx_debug_adj3_tail_words(C.byref(off_d), C.byref(off_s)) == (1 if tail else 0)
    net = make_net(pa, dev, p)
    pe = engine.params_cached(*pa.odenet.params_of(net))
    y0d, td = torch.from_numpy(y0).to(dev), torch.from_numpy(t).to(dev).contiguous()
    Gd = torch.from_numpy(np.ascontiguousarray(G.transpose(1, 0, 2))).to(dev)
    sol, st, _, _ = engine.solve_forward(pe, y0d, td, "dopri5", _lib.CTRL_PER_TRAJECTORY, 1e-7, 1e-9, True, 2)
    engine.forget_workspaces()
    ws, _ = engine._workspace(_lib.OP_ADJOINT, N, H, B, T, dev)
    ws[off_s.value: off_s.value + 4].zero_()      # (the header's words; the solve's own fill follows)
    adj, gr, st2, _, ns = engine.solve_adjoint(pe, td, sol, Gd, "dopri5", _lib.CTRL_PER_TRAJECTORY, 1e-7, 1e-9, True, 2,
                                               want_grads=want_grads)
    assert int(st.max()) == 0 and int(st2.max()) == 0
    TG, _ = plan_of(N, H, B, T)
    deferred = ws[off_d.value: off_d.value + 4 * TG].cpu().numpy().view(np.uint32).tolist()
    served = int(ws[off_s.value: off_s.value + 4].cpu().numpy().view(np.uint32)[0])
    grads = None
    if gr is not None:
        grads = {k: getattr(gr, k).cpu().numpy().copy() for k in KEYS}
    return adj.cpu().numpy(), grads, ns.cpu().numpy(), deferred, served


def check_vs_oracle(adj, grads, adj_ref, gr_ref, tag):
    for name, fig in [("adj_y0", grad_err(adj, adj_ref, tag))] + \
                     [(k, grad_err(grads[k].reshape(gr_ref[k].shape), gr_ref[k], tag)) for k in KEYS]:
        print("%s %s: %.3e" % (tag, name, fig))
        assert fig < TOL_DOPRI_GRAD, (tag, name, fig)


@pytest.mark.parametrize("N,H,B", SHAPES)
def test_every_group_defers_its_single_step(pa, dev, oracle, monkeypatch, N, H, B):
    p, y0, t, G, adj_ref, gr_ref = problem(oracle, N, H, B, "one")
    TG, _ = plan_of(N, H, B, 2)
    if B == 80:
        assert TG >= 2
    adj, gr, ns, deferred, served = solve(pa, dev, monkeypatch, p, y0, t, G, tail=True)
    assert (ns == 1).all(), ns.tolist()
    assert deferred == [1] * TG and served == TG, (deferred, served)      # the tail path ran, for every group
    check_vs_oracle(adj, gr, adj_ref, gr_ref, "tail %d/%d/%d" % (N, H, B))
    assert (gr["g"][p["g"] <= 0] == 0.0).all()
    adj2, gr2, _, deferred2, served2 = solve(pa, dev, monkeypatch, p, y0, t, G, tail=True)
    assert deferred2 == deferred and served2 == served
    assert same_bits(adj, adj2) and all(same_bits(gr[k], gr2[k]) for k in KEYS)   # deterministic
    adj0, gr0, ns0, deferred0, served0 = solve(pa, dev, monkeypatch, p, y0, t, G, tail=False)
    assert (ns0 == 1).all() and deferred0 == [0] * TG and served0 == 0
    check_vs_oracle(adj0, gr0, adj_ref, gr_ref, "in-kernel %d/%d/%d" % (N, H, B))
    assert (gr0["g"][p["g"] <= 0] == 0.0).all()


@pytest.mark.parametrize("N,H,B", SHAPES)
def test_a_group_of_several_steps_keeps_its_partial(pa, dev, oracle, monkeypatch, N, H, B):
    """the last batch group integrates over [0, 1] (several steps: it runs its visits itself and the tail launch adds its
    partial), the groups in front of it defer; with one batch group the launch defers nothing"""
    p, y0, t, G, adj_ref, gr_ref = problem(oracle, N, H, B, "mixed")
    TG, Bt = plan_of(N, H, B, 2)
    adj, gr, ns, deferred, served = solve(pa, dev, monkeypatch, p, y0, t, G, tail=True)
    long_rows = np.arange(B) >= (TG - 1) * Bt
    assert (ns[long_rows] > 1).all() and (ns[~long_rows] == 1).all(), ns.tolist()
    assert deferred == [1] * (TG - 1) + [0] and served == TG - 1, (deferred, served)
    check_vs_oracle(adj, gr, adj_ref, gr_ref, "mixed tail %d/%d/%d" % (N, H, B))
    assert (gr["g"][p["g"] <= 0] == 0.0).all()
    adj2, gr2, _, _, _ = solve(pa, dev, monkeypatch, p, y0, t, G, tail=True)
    assert same_bits(adj, adj2) and all(same_bits(gr[k], gr2[k]) for k in KEYS)
    adj0, gr0, _, deferred0, _ = solve(pa, dev, monkeypatch, p, y0, t, G, tail=False)
    assert deferred0 == [0] * TG
    check_vs_oracle(adj0, gr0, adj_ref, gr_ref, "mixed in-kernel %d/%d/%d" % (N, H, B))
    assert same_bits(adj[long_rows], adj0[long_rows])      # the group that did not defer: the same path, the same bits


@pytest.mark.parametrize("N,H,B", SHAPES)
def test_three_time_points_defer_nothing(pa, dev, oracle, monkeypatch, N, H, B):
    p, y0, t, G, adj_ref, gr_ref = problem(oracle, N, H, B, "three")
    TG, _ = plan_of(N, H, B, 3)
    adj, gr, ns, deferred, served = solve(pa, dev, monkeypatch, p, y0, t, G, tail=True)
    assert (ns >= 2).all() and deferred == [0] * TG and served == 0, (ns.tolist(), deferred, served)
    check_vs_oracle(adj, gr, adj_ref, gr_ref, "T=3 tail %d/%d/%d" % (N, H, B))
    adj0, gr0, _, _, _ = solve(pa, dev, monkeypatch, p, y0, t, G, tail=False)
    check_vs_oracle(adj0, gr0, adj_ref, gr_ref, "T=3 in-kernel %d/%d/%d" % (N, H, B))
    assert same_bits(adj, adj0)


@pytest.mark.parametrize("N,H,B", SHAPES)
def test_without_parameter_gradients_nothing_is_deferred(pa, dev, oracle, monkeypatch, N, H, B):
    p, y0, t, G, adj_ref, _ = problem(oracle, N, H, B, "one")
    adj, gr, ns, _, served = solve(pa, dev, monkeypatch, p, y0, t, G, tail=True, want_grads=False)
    assert gr is None and (ns == 1).all() and served == 0
    fig = grad_err(adj, adj_ref, "no grads %d/%d/%d" % (N, H, B))
    print("no grads adj_y0: %.3e" % fig)
    assert fig < TOL_DOPRI_GRAD
    adj0, _, _, _, _ = solve(pa, dev, monkeypatch, p, y0, t, G, tail=False, want_grads=False)
    assert same_bits(adj, adj0)
