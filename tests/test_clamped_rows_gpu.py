"""Perturbation time courses on the MI355X: the `clamp=` keyword of `odeint` / `odeint_adjoint` / `odeint_per_sample` -- a
set of held genes per trajectory ROW, forward and adjoint (phx_odeint_clamped_rows,
phx_odeint_adjoint_backward_clamped_rows: the CLAMP forms of k1_solve_fwd3 and k1_solve_adj3; everything else the grouped
path) -- against the model the clamp is defined by: the same parameters with g zeroed on the row's set, solved by the CPU
oracle once per distinct set on the rows of that set, parameter gradients summed over the sets in float64.  Tolerances are
the project's (tests/test_gpu_parity.py).  Run with `-m gpu`; every test prints the figures it measured before it asserts.

The forms each shape (N, H, B) of test 1 runs, as planned for 256 CUs (asserted through phx_debug_clamped_rows_plan), the
same for both kernels:
    (96, 8, 5)      HALF, SPLIT      one partial tile
    (350, 30, 37)   HALF             three tiles: sets differ between neighbouring rows and across rows 15 / 16
    (96, 44, 5)     full, SPLIT      full last hidden tile
    (350, 44, 150)  full             several batch groups, the last one not filled ((350, 40, 150) is a HALF form)
Measured on an MI355X, test 1: sol <= 4.6e-6 (bar 1e-5), held columns drift exactly 0, adj_y0 <= 1.31e-5, the six parameter
gradients <= 4.2e-6 (bar 2.5e-5); test 2: exactly 0 and 0, against -6.8e-5 and 2.7e-2 with one row free.
"""
import ctypes as C

import numpy as np
import pytest
import torch

from conftest import grad_err, relerr
from test_gpu_parity import KEYS, TOL_DOPRI, TOL_DOPRI_GRAD, TOL_FIXED, grads_of, make_net, onet_of, rand_params, zero_grads

pytestmark = pytest.mark.gpu

T = 3


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "these tests need the MI355X"
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def pa():
    import phoenix_amd
    return phoenix_amd


def _zeroed(p, held):
    q = dict(p)
    q["g"] = p["g"].copy()
    q["g"][list(held)] = 0.0
    return q


def _plan(op, N, H, B):
    from phoenix_amd import _lib
    plan = (C.c_int * 8)()
    assert _lib.load().phx_debug_clamped_rows_plan(op, N, H, B, T, plan) == 1
    return list(plan)      # kernel, HALF, SPLIT, rows per launch, launches, TG, G, ntg


def _problem(N, H, B, seed, scale=1.0):
    """parameters as in the knockout tests, y0 [B, N], a time grid per sample (T = 3, so that the backward solve takes the
    jump a += grad_y[i - 1]) and cotangents on every output time"""
    p = rand_params(N, H, seed=seed, std=0.6 / np.sqrt(N))
    rs = np.random.RandomState(seed + 1)
    y0 = ((rs.rand(B, N).astype(np.float32) - 0.25) * (0.6 + 0.2 * (np.arange(B) % 4))[:, None]).astype(np.float32)
    t = 0.05 * (np.arange(B) % 5)[:, None] + np.cumsum(np.concatenate([np.zeros((B, 1)), rs.uniform(0.2, 0.5, (B, T - 1))], 1), 1)
    G = (rs.randn(B, T, N) * scale).astype(np.float32)
    return p, y0, t, G


def _distinct_sets(oracle, p, y0):
    """six sets: the empty one, widths 1 .. 4, genes at 0, 15 / 16, 31 / 32 and N - 1, a gene with g <= 0, and "m", the
    gene with a positive multiplier whose slope at y0 is largest; returns them and m"""
    N = p["g"].shape[0]
    pos, neg = np.flatnonzero(p["g"] > 0), np.flatnonzero(p["g"] <= 0)
    f = np.abs(oracle.rhs(onet_of(oracle, p), y0)).reshape(-1, N).max(axis=0)
    m = int(pos[np.argmax(f[pos])])
    ng = int(neg[len(neg) // 2])
    sets = [(), (m,), (15, 16), (0, 31, 32), tuple(sorted({m, ng, N - 1, 16})), (N - 1,)]
    assert [len(s) for s in sets] == [0, 1, 2, 3, 4, 1]
    return sets, m


def _truth(oracle, p, y0, t, G, sets, method="dopri5"):
    """the oracle once per distinct set, on the rows of that set, with g zeroed on the set: sol [B,T,N], adj_y0 [B,N] and
    the six parameter gradients summed over the sets in float64"""
    B, N = y0.shape
    sol, adj = np.zeros((B, t.shape[1], N), np.float32), np.zeros((B, N), np.float32)
    gr = None
    for held in sorted(set(sets)):
        rows = [b for b in range(B) if sets[b] == held]
        onet = onet_of(oracle, _zeroed(p, held))
        ref = oracle.odeint_per_sample(onet, y0[rows], t[rows], method=method)
        a, g = oracle.adjoint_backward_per_sample(onet, t[rows], ref, G[rows], method=method, theta_in_norm=True)
        sol[rows], adj[rows] = ref, np.asarray(a).reshape(len(rows), N)
        gr = ({k: np.asarray(g[k], np.float64).copy() for k in KEYS} if gr is None
              else {k: gr[k] + np.asarray(g[k], np.float64) for k in KEYS})
    return sol, adj, gr


def _run(pa, dev, net, y0, t, G, clamp, fn=None, **kw):
    """sol [B,T,N], adj_y0 [B,N] and the parameter gradients of sum(G * fn(net, y0, t, clamp=clamp)) through the public
    entry point; t [B,T] or [T]"""
    zero_grads(net)
    B, N = y0.shape
    y0t = torch.from_numpy(y0).to(dev).reshape(B, 1, N).requires_grad_(True)
    sol = (fn or pa.odeint_adjoint)(net, y0t, torch.from_numpy(t).to(dev), clamp=clamp, **kw)
    Tn = sol.shape[0]
    (sol * torch.from_numpy(G.transpose(1, 0, 2).reshape(Tn, B, 1, N).copy()).to(dev)).sum().backward()
    torch.cuda.synchronize()
    return (sol.detach().cpu().numpy().reshape(Tn, B, N).transpose(1, 0, 2), y0t.grad.cpu().numpy().reshape(B, N),
            grads_of(net))


def _check(tag, got, want, sets, y0, tol_y, tol_g):
    sol, adj, gr = got
    rsol, radj, rgr = want
    e = {"sol": relerr(sol, rsol), "adj_y0": grad_err(adj, radj, tag)}
    hold = 0.0
    for b, held in enumerate(sets):
        for k in held:
            hold = max(hold, float(np.abs(sol[b, :, k] - y0[b, k]).max()) / max(float(np.abs(rsol).max()), 1e-30))
    e.update({k: grad_err(gr[k], rgr[k], tag + " " + k) for k in KEYS})
    print("%s: %s, held columns drift %.3e" % (tag, ", ".join("%s %.3e" % kv for kv in e.items()), hold))
    assert e["sol"] < tol_y and hold < tol_y
    for k in ["adj_y0"] + list(KEYS):
        assert e[k] < tol_g, (tag, k, e[k])


# --------------------------------------------------------------------------- 1. every kernel form against the oracle
SHAPES = [(96, 8, 5, (1, 1)), (350, 30, 37, (1, 0)), (96, 44, 5, (0, 1)), (350, 44, 150, (0, 0))]


@pytest.mark.parametrize("N,H,B,form", SHAPES)
def test_clamped_rows_equal_the_per_row_model_with_zeroed_multipliers(pa, dev, oracle, N, H, B, form):
    from phoenix_amd import _lib
    for op in (_lib.OP_ODEINT, _lib.OP_ADJOINT):
        plan = _plan(op, N, H, B)
        assert plan[0] == 3 and tuple(plan[1:3]) == form and plan[4] == 1, plan
    p, y0, t, G = _problem(N, H, B, seed=N + H + B)
    distinct, m = _distinct_sets(oracle, p, y0)
    sets = [distinct[b % len(distinct)] for b in range(B)]
    assert sets[15 % B] != sets[16 % B] or B < 17
    want = _truth(oracle, p, y0, t, G, sets)
    # conditions on the inputs, from the oracle alone: an ignored mask in either kernel could not pass
    free = _truth(oracle, p, y0, t, G, [()] * B)
    moved = max(float(np.abs(free[0][b, :, k] - want[0][b, :, k]).max()) for b in range(B) for k in sets[b]) / float(np.abs(want[0]).max())
    d_adj, d_wa = relerr(free[1], want[1]), relerr(free[2]["Wa"], want[2]["Wa"])
    print("the unclamped oracle moves a held gene by %.3e of the trajectory scale; clamped vs unclamped adj_y0 %.3e, dWa %.3e"
          % (moved, d_adj, d_wa))
    assert moved > 100 * TOL_DOPRI and d_adj > 100 * TOL_DOPRI_GRAD and d_wa > 100 * TOL_DOPRI_GRAD
    net = make_net(pa, dev, p)
    g_obj, g_before = net.gene_multipliers, net.gene_multipliers.detach().clone()
    got = _run(pa, dev, net, y0, t, G, sets)
    assert net.gene_multipliers is g_obj and torch.equal(net.gene_multipliers.detach(), g_before)
    # the engine's own unclamped odeint_adjoint on a zeroed module, set by set: how many rows agree bit for bit
    znet, same = make_net(pa, dev, p), 0
    for held in sorted(set(sets)):
        rows = [b for b in range(B) if sets[b] == held]
        with torch.no_grad():
            znet.gene_multipliers.copy_(torch.from_numpy(_zeroed(p, held)["g"]).reshape(1, N))
        own = _run(pa, dev, znet, y0[rows], t[rows], G[rows], None)
        same += sum(bool(np.array_equal(got[0][b], own[0][i]) and np.array_equal(got[1][b], own[1][i])) for i, b in enumerate(rows))
    print("rows equal to the engine's unclamped odeint_adjoint on the zeroed module, bit for bit (sol and adj_y0): %d of %d" % (same, B))
    _check("(%d, %d, %d)" % (N, H, B), got, want, sets, y0, TOL_DOPRI, TOL_DOPRI_GRAD)
    # forward only, and the tensor form of the list: the same trajectories
    width = max(len(s) for s in sets)
    lst = torch.tensor([list(s) + [-1] * (width - len(s)) for s in sets])
    with torch.no_grad():
        fwd = pa.odeint_per_sample(net, torch.from_numpy(y0).to(dev).reshape(B, 1, N), torch.from_numpy(t).to(dev), clamp=lst,
                                   adjoint=False)
    assert np.array_equal(fwd.cpu().numpy().reshape(T, B, N).transpose(1, 0, 2), got[0])


# --------------------------------------------------------------------------- 2. the quadrature mask on its own
def test_a_gene_held_in_every_row_gets_exactly_no_gradient(pa, dev, oracle):
    N, H, B = 96, 8, 5
    p, y0, t, G = _problem(N, H, B, seed=7)
    _, m = _distinct_sets(oracle, p, y0)
    net = make_net(pa, dev, p)
    _, _, gr = _run(pa, dev, net, y0, t, G, [m] * B)
    assert np.array_equal(gr["g"][m], np.float32(0.0)) and np.array_equal(gr["Wa"][m], np.zeros(2 * H, np.float32))
    assert torch.equal(net.gene_multipliers.grad.reshape(-1)[m], torch.zeros((), device=dev))
    assert torch.equal(net.net_alpha_combine.linear_out.weight.grad[m], torch.zeros(2 * H, device=dev))
    assert np.abs(gr["g"]).max() > 0 and np.abs(gr["Wa"]).max() > 0
    _, _, gr1 = _run(pa, dev, net, y0, t, G, [m] * (B - 1) + [-1])            # all rows but one
    print("gene %d held in every row: dg %g, max |dWa row| %g; in all rows but one: dg %g, max |dWa row| %g"
          % (m, gr["g"][m], np.abs(gr["Wa"][m]).max(), gr1["g"][m], np.abs(gr1["Wa"][m]).max()))
    assert gr1["g"][m] != 0 and np.abs(gr1["Wa"][m]).max() > 0


# --------------------------------------------------------------------------- 3. neighbours
def test_one_rows_set_leaves_the_other_rows_alone(pa, dev, oracle):
    """Rows of a per-trajectory launch are bitwise independent in the unclamped kernels (measured on the MI355X by changing
    one row's y0 at this shape: every other row of sol and adj_y0 kept its bits), so the other rows must keep theirs when
    one row's set changes."""
    N, H, B = 350, 30, 37
    p, y0, t, G = _problem(N, H, B, seed=21)
    distinct, m = _distinct_sets(oracle, p, y0)
    sets = [distinct[b % len(distinct)] for b in range(B)]
    net = make_net(pa, dev, p)
    base = _run(pa, dev, net, y0, t, G, sets)
    for row, held in ((17, (m, 3)), (0, (m,)), (36, (5, 349)), (16, ())):
        assert sets[row] != held
        other = _run(pa, dev, net, y0, t, G, sets[:row] + [held] + sets[row + 1:])
        keep = [b for b in range(B) if b != row]
        same = [bool(np.array_equal(base[i][keep], other[i][keep])) for i in (0, 1)]
        diff = [relerr(other[i][keep], base[i][keep]) for i in (0, 1)]
        print("row %d: the other rows' sol / adj_y0 bitwise equal: %s (relerr %.3e / %.3e); the row itself moved by %.3e"
              % (row, same, diff[0], diff[1], relerr(other[0][row], base[0][row])))
        assert all(same)
        assert not np.array_equal(base[0][row], other[0][row])


# --------------------------------------------------------------------------- 4. a batch the chunk driver splits
def test_a_batch_of_several_launches_offsets_the_list_with_the_rows(pa, dev, oracle):
    from phoenix_amd import _lib
    N, H, B = 96, 8, 65537          # the smallest batch at (96, 8) that does not fit one launch: 16 x 4096 rows + 1
    for op in (_lib.OP_ODEINT, _lib.OP_ADJOINT):
        assert _plan(op, N, H, B - 1)[4] == 1
        plan = _plan(op, N, H, B)
        assert plan[3] == 4096 and plan[4] == 17, plan
    p, y0, t, G = _problem(N, H, B, seed=5)
    distinct, _ = _distinct_sets(oracle, p, y0[:64])
    sets = [distinct[(b + b // 4096) % len(distinct)] for b in range(B)]
    net = make_net(pa, dev, p)
    sol, adj, _ = _run(pa, dev, net, y0, t, G, sets)
    rows = sorted({0, B - 1} | {k * 4096 - 1 for k in range(1, 17)} | {k * 4096 for k in range(1, 17)})
    rsol, radj, _ = _truth(oracle, p, y0[rows], t[rows], G[rows], [sets[b] for b in rows])
    e_y = np.abs(sol[rows] - rsol).reshape(len(rows), -1).max(1) / np.abs(rsol).max()
    e_a = np.abs(adj[rows] - radj).max(1) / np.abs(radj).max()
    print("rows on both sides of every split: worst sol %.3e (row %d), worst adj_y0 %.3e (row %d)"
          % (e_y.max(), rows[int(e_y.argmax())], e_a.max(), rows[int(e_a.argmax())]))
    assert e_y.max() < TOL_DOPRI and e_a.max() < TOL_DOPRI_GRAD
    for b in rows:
        for k in sets[b]:
            assert np.abs(sol[b, :, k] - y0[b, k]).max() < TOL_DOPRI * np.abs(rsol).max(), (b, k)


# --------------------------------------------------------------------------- 5. the grouped path
def _grouped_inputs(oracle, N, H, B, seed):
    p, y0, t, G = _problem(N, H, B, seed=seed, scale=1.0 / (B * N))
    distinct, m = _distinct_sets(oracle, p, y0)
    sets = [distinct[1], distinct[0], distinct[4], distinct[1], distinct[2]]
    return p, y0, t, G, sets


@pytest.mark.parametrize("case", ["H56", "rk4", "v0"])
def test_grouped_path_against_the_oracle(pa, dev, oracle, monkeypatch, case):
    from phoenix_amd import _lib, engine
    N, B = 96, 5
    H = 56 if case == "H56" else 8
    method = "rk4" if case == "rk4" else "dopri5"
    if case == "v0":
        monkeypatch.setenv("PHX_ENGINE", "v0")
    for op in (_lib.OP_ODEINT, _lib.OP_ADJOINT):
        assert engine.clamped_rows_plan_exists(op, N, H, B, T, method) == 0       # no kernel: the grouped path
    p, y0, t, G, sets = _grouped_inputs(oracle, N, H, B, seed=31)
    want = _truth(oracle, p, y0, t, G, sets, method)
    net = make_net(pa, dev, p)
    g_obj, g_before = net.gene_multipliers, net.gene_multipliers.detach().clone()
    got = _run(pa, dev, net, y0, t, G, sets, method=method)
    assert net.gene_multipliers is g_obj and torch.equal(net.gene_multipliers.detach(), g_before)
    fixed = method != "dopri5"
    _check(case, got, want, sets, y0, TOL_FIXED if fixed else TOL_DOPRI, TOL_FIXED if fixed else TOL_DOPRI_GRAD)


@pytest.mark.parametrize("h", [None, 0.125])
def test_grouped_path_backpropagates_through_the_steps(pa, dev, oracle, h):
    """`odeint` with rk4 (one step per interval, and options["step_size"]): the discrete adjoint, which the oracle does not
    have -- the truth is the float64 torch arbiter of tests/test_backprop_gpu.py on the zeroed parameters, set by set"""
    from test_backprop_gpu import arbiter
    N, H, B = 96, 8, 5
    p, y0, _, G, sets = _grouped_inputs(oracle, N, H, B, seed=33)
    t = np.array([0.0, 0.4, 0.9])
    Gt = G.transpose(1, 0, 2).copy()
    sol, adj, gr = np.zeros((B, T, N)), np.zeros((B, N)), {k: 0.0 for k in KEYS}
    for held in sorted(set(sets)):
        rows = [b for b in range(B) if sets[b] == held]
        ref = arbiter(pa, _zeroed(p, held), dev, torch.float64, y0[rows], t, Gt[:, rows].copy(), "rk4", h)
        sol[rows], adj[rows] = ref["sol"].transpose(1, 0, 2), ref["grad_y0"]
        gr = {k: gr[k] + ref["grad_" + k] for k in KEYS}
    net = make_net(pa, dev, p)
    g_obj, g_before = net.gene_multipliers, net.gene_multipliers.detach().clone()
    opts = {"batch_control": "per_trajectory"}
    if h:
        opts["step_size"] = h
    got = _run(pa, dev, net, y0, t, G, sets, fn=pa.odeint, method="rk4", options=opts)
    assert net.gene_multipliers is g_obj and torch.equal(net.gene_multipliers.detach(), g_before)
    _check("odeint rk4 h=%s" % h, got, (sol, adj, gr), sets, y0, TOL_FIXED, TOL_FIXED)


def test_grouped_path_and_kernel_path_agree(pa, dev, oracle, monkeypatch):
    from phoenix_amd import engine
    N, H, B = 96, 8, 5
    p, y0, t, G, sets = _grouped_inputs(oracle, N, H, B, seed=35)
    net = make_net(pa, dev, p)
    kern = _run(pa, dev, net, y0, t, G, sets)
    monkeypatch.setattr(engine, "clamped_rows_plan_exists", lambda *a, **k: 0)
    grouped = _run(pa, dev, net, y0, t, G, sets)
    e = {"sol": relerr(kern[0], grouped[0]), "adj_y0": relerr(kern[1], grouped[1])}
    e.update({k: relerr(kern[2][k], grouped[2][k]) for k in KEYS})
    print("kernel path against grouped path: " + ", ".join("%s %.3e" % kv for kv in e.items()))
    assert all(v < TOL_DOPRI_GRAD for v in e.values()), e


# --------------------------------------------------------------------------- 6. error status
def test_a_failing_clamped_row_raises_from_backward(pa, dev):
    """the status path: a clamped row that exhausts max_num_steps surfaces as the reference's AssertionError from
    backward(), like an unclamped one; under no_grad the forward raises at once"""
    N, H, B = 350, 30, 6
    p = rand_params(N, H, seed=9, std=0.5 / np.sqrt(N))
    net = make_net(pa, dev, p)
    y0 = torch.rand(B, 1, N, device=dev)
    t = torch.tensor([[0.0, 50.0]] * B, device=dev)
    clamp = [3, -1, (5, 6), -1, -1, 7]
    yg = y0.clone().requires_grad_(True)
    sol = pa.odeint_adjoint(net, yg, t, options={"max_num_steps": 2}, clamp=clamp)
    with pytest.raises(AssertionError, match="max_num_steps"):
        sol.sum().backward()
    with torch.no_grad():
        with pytest.raises(AssertionError, match="max_num_steps"):
            pa.odeint_adjoint(net, y0, t, options={"max_num_steps": 2}, clamp=clamp)
    # and the engine is in order afterwards
    yg = y0.clone().requires_grad_(True)
    sol = pa.odeint_adjoint(net, yg, torch.tensor([[0.0, 0.5]] * B, device=dev), clamp=clamp)
    sol.sum().backward()
    assert torch.isfinite(yg.grad).all() and torch.isfinite(sol).all()
