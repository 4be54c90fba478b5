"""Terminal tiles of k1_solve_fwd3 (phx_mfma_fwd3.inc): where the candidate step of every running trajectory of a tile
reaches its last output time, the last-stage sweep writes the dense output from registers and the tile has no accept pass.
Every case is solved with the fold on and off (`PHX_V3_TERM=0`: every tile ends its steps with the accept pass) -- `sol`,
`status`, `nfe`, `nsteps` must be equal bit for bit, the sign of a zero aside -- and the fold-on trajectories are held to
the CPU oracle at the dopri5 bar of tests/test_gpu_parity.py.  N = 70 is three gene blocks, the last one partial; H = 40
takes the HALF instantiations, H = 48 the full ones.  On the MI355X; run with `-m gpu`."""
import numpy as np
import pytest
import torch

from conftest import relerr
from test_gpu_parity import TOL_DOPRI, make_net, onet_of, rand_params

pytestmark = pytest.mark.gpu

N = 70
T_END = 0.0051        # the flagship interval: the first candidate step covers it
T_LONG = 0.3          # case (c): several steps on the same problem (asserted on the oracle)
T_REJECT = 1e-6       # case (d): far below any initial step


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "these tests need the MI355X"
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def pa():
    import phoenix_amd
    return phoenix_amd


def dense_params(H, seed=7, std=0.05):
    """dense N(0, std) factors and positive gene multipliers, as bench.make_problem draws them"""
    return rand_params(N, H, seed=seed, std=std, neg=0.0)


def states(B, seed=11):
    r = np.random.RandomState(seed)
    return np.clip(r.randn(B, N) * 0.15 + 0.5, 0.03, 1.07).astype(np.float32)


def rejecting_states(oracle, onet, n, seed0=0):
    """n states whose first candidate step towards T_REJECT the CPU oracle rejects: 8 evaluations are one attempt (two
    for the initial step, six stages), every further attempt costs six, so nfe >= 14 at an end time far below the
    initial step says that the first -- terminal -- candidate was not accepted"""
    rows, seed = [], seed0
    while len(rows) < n:
        assert seed < seed0 + 200, "no rejected first step found: case (d) would lose its coverage"
        y = states(1, seed=1000 + seed)
        seed += 1
        try:
            _, nfe, _ = oracle.odeint(onet, y, np.array([0.0, T_REJECT], np.float32), return_stats=True)
        except Exception:      # the oracle gave up on this state
            continue
        if nfe >= 14:
            rows.append(y[0])
    return np.stack(rows)


def same_bits(a, b):
    """equal bit for bit, except that +0 and -0 count as equal"""
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    if a.dtype != np.float32:
        return a.shape == b.shape and bool((a == b).all())
    return a.shape == b.shape and bool(((a.view(np.uint32) == b.view(np.uint32)) | ((a == 0) & (b == 0))).all())


def solve_on_and_off(pa, dev, monkeypatch, p, y0, t, shared=False):
    """engine.solve_forward with the fold on and off; asserts the bitwise equality and returns the fold-on results:
    sol [B, T, N], status, nfe, nsteps.  t: [T] (shared control) or [B, T] (a controller and a time row per trajectory)"""
    from phoenix_amd import _lib, engine
    net = make_net(pa, dev, p)
    pe = engine.params_cached(*pa.odenet.params_of(net))
    y0d, td = torch.from_numpy(y0).to(dev), torch.from_numpy(np.asarray(t, np.float32)).to(dev).contiguous()
    control = _lib.CTRL_SHARED if shared else _lib.CTRL_PER_TRAJECTORY
    B, T = y0.shape[0], td.shape[-1]
    assert _lib.load().phx_debug_forward_kernel_m(N, p["Ws"].shape[0], B, T, control, _lib.METHODS["dopri5"]) == 3

    def run():
        sol, st, nfe, ns = engine.solve_forward(pe, y0d, td, "dopri5", control, 1e-7, 1e-9, not shared, 2)
        return sol.cpu().numpy().transpose(1, 0, 2), st.cpu().numpy(), nfe.cpu().numpy(), ns.cpu().numpy()

    monkeypatch.delenv("PHX_V3_TERM", raising=False)
    on = run()
    monkeypatch.setenv("PHX_V3_TERM", "0")
    off = run()
    monkeypatch.delenv("PHX_V3_TERM")
    for name, a, b in zip(("sol", "status", "nfe", "nsteps"), on, off):
        assert same_bits(a, b), name
    return on


@pytest.mark.parametrize("H", [40, 48])
@pytest.mark.parametrize("B", [5, 19, 80])
def test_a_single_terminal_step(pa, dev, oracle, monkeypatch, H, B):
    """B = 5: the waves of the tile split its gene blocks; 19: two tiles, padding rows; 80: more than one batch group"""
    p, y0 = dense_params(H), states(B)
    t = np.tile(np.array([0.0, T_END], np.float32), (B, 1))
    sol, st, nfe, ns = solve_on_and_off(pa, dev, monkeypatch, p, y0, t)
    assert (st == 0).all() and (nfe == 8).all() and (ns == 1).all()
    assert relerr(sol, oracle.odeint_per_sample(onet_of(oracle, p), y0, t, method="dopri5")) < TOL_DOPRI


@pytest.mark.parametrize("H", [40, 48])
@pytest.mark.parametrize("B", [5, 19])
def test_b_several_output_times_inside_the_terminal_step(pa, dev, oracle, monkeypatch, H, B):
    p, y0 = dense_params(H), states(B)
    t = np.tile(np.array([0.0, 0.002, 0.004, T_END], np.float32), (B, 1))
    sol, st, nfe, ns = solve_on_and_off(pa, dev, monkeypatch, p, y0, t)
    assert (st == 0).all() and (nfe == 8).all()
    assert relerr(sol, oracle.odeint_per_sample(onet_of(oracle, p), y0, t, method="dopri5")) < TOL_DOPRI


@pytest.mark.parametrize("H", [40, 48])
def test_c_a_tile_of_terminal_and_continuing_trajectories(pa, dev, oracle, monkeypatch, H):
    """one tile: the even rows end inside their first candidate step, the odd ones take several steps (the tile is not
    terminal before they near their end; the finished rows' state is not written back any more)"""
    B = 16
    p, y0 = dense_params(H), states(B)
    onet = onet_of(oracle, p)
    t = np.array([[0.0, T_END if b % 2 == 0 else T_LONG] for b in range(B)], np.float32)
    for b in range(1, B, 2):      # raises unless the oracle's status is OK
        assert oracle.odeint(onet, y0[b:b + 1], t[b], return_stats=True)[2] > 1
    sol, st, nfe, ns = solve_on_and_off(pa, dev, monkeypatch, p, y0, t)
    assert (st == 0).all() and (ns[0::2] == 1).all() and (ns[1::2] > 1).all()
    assert relerr(sol, oracle.odeint_per_sample(onet, y0, t, method="dopri5")) < TOL_DOPRI


@pytest.mark.parametrize("H", [40, 48])
@pytest.mark.parametrize("B", [3, 19])
def test_d_a_rejected_terminal_candidate(pa, dev, oracle, monkeypatch, H, B):
    """factors of unit size: the first candidate step, which reaches the end time, fails the error test.  The terminal
    sweep has written output rows for it; the trajectory must repeat the step from untouched tiles and the accepted
    step's rows replace them.  B = 19: every other row is one of case (a)'s kind on the same problem."""
    p = dense_params(H, seed=100, std=1.0)
    onet = onet_of(oracle, p)
    hard = [b for b in range(B)] if B == 3 else [b for b in range(B) if b % 2 == 0]
    y0 = states(B, seed=5)
    y0[hard] = rejecting_states(oracle, onet, len(hard))
    t = np.tile(np.array([0.0, T_END], np.float32), (B, 1))
    t[hard, 1] = T_REJECT
    for b in hard:     # the precondition itself, so that the coverage cannot silently be lost
        assert oracle.odeint(onet, y0[b:b + 1], t[b], return_stats=True)[1] >= 14
    ref = oracle.odeint_per_sample(onet, y0, t, method="dopri5")
    sol, st, nfe, ns = solve_on_and_off(pa, dev, monkeypatch, p, y0, t)
    assert (st == 0).all() and (nfe[hard] >= 14).all() and (ns[hard] >= 2).all()
    assert relerr(sol, ref) < TOL_DOPRI


@pytest.mark.parametrize("H", [40, 48])
def test_e_shared_control(pa, dev, oracle, monkeypatch, H):
    B = 19
    p, y0 = dense_params(H), states(B)
    t = np.array([0.0, T_END], np.float32)
    sol, st, nfe, ns = solve_on_and_off(pa, dev, monkeypatch, p, y0, t, shared=True)
    assert (st == 0).all() and (nfe == 8).all()
    assert relerr(sol.transpose(1, 0, 2), oracle.odeint(onet_of(oracle, p), y0, t)) < TOL_DOPRI


@pytest.mark.parametrize("H", [40, 48])
def test_e_call_batched_launch(pa, dev, oracle, monkeypatch, H):
    """three odeint calls of five rows in one launch (the CALLS instantiations): a controller per call"""
    from phoenix_amd import _lib
    K, B = 3, 5
    p = dense_params(H)
    net = make_net(pa, dev, p)
    y0s = np.stack([states(B, seed=20 + k) for k in range(K)]).reshape(K, B, 1, N)
    y0d, td = torch.from_numpy(y0s).to(dev), torch.tensor([0.0, T_END], device=dev)
    assert _lib.load().phx_debug_calls_grids_kernel_m(N, H, B * K, 2, K, _lib.METHODS["dopri5"]) == 3
    monkeypatch.delenv("PHX_V3_TERM", raising=False)
    on = pa.odeint_calls(net, y0d, td, method="dopri5").cpu().numpy()
    monkeypatch.setenv("PHX_V3_TERM", "0")
    off = pa.odeint_calls(net, y0d, td, method="dopri5").cpu().numpy()
    monkeypatch.delenv("PHX_V3_TERM")
    assert on.shape == (K, 2, B, 1, N) and same_bits(on, off)
    onet = onet_of(oracle, p)
    for k in range(K):
        ref, nfe, _ = oracle.odeint(onet, y0s[k], np.array([0.0, T_END], np.float32), return_stats=True)
        assert nfe == 8
        assert relerr(on[k], ref) < TOL_DOPRI, k
