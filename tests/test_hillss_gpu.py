"""GPU tests of the Hill simulator's steady states (phx_hill_steady; `HillSystem.steady_states` / `knockout_steady_states`,
`steady_state_recovery`) against the float64 fixed points of `steady_states_reference`, under the bound
tests/test_steady_gpu.py derives: with x* the reference's fixed point, kappa = ||J^-1||_inf of the float64 Jacobian on the
moving genes at x* and r32 the largest difference between `rates_reference` in float32 and in float64 at the result,
    the float64 residual of the result <= tol + r32   and   |result - x*| <= 2 kappa (tol + r32).
Systems, states and references: tests/test_hillss_cpu.py, whose reference results (all rows converged) these rest on."""
import numpy as np
import pytest
import torch

from test_hillko_cpu import descendants, gene_with_descendants
from test_hillss_cpu import case, dense_jacobian, moving, reference
from test_simulator_cpu import synthetic_network, synthetic_states

pytestmark = pytest.mark.gpu
TOL = 1e-5
CASES = ("syn12", "syn40", "syn96", "g11")


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "these tests need the MI355X"
    return torch.device("cuda:0")


_GPU = {}


def on_device(name, dev):
    """(system on the device, x0 tensor) of a case of tests/test_hillss_cpu.py"""
    from phoenix_amd.simulator import HillSystem
    if name not in _GPU:
        sys_, x0, _, _ = case(name)
        _GPU[name] = (HillSystem(sys_.names, sys_.expressions, device=dev), torch.from_numpy(x0).to(dev))
    return _GPU[name]


def rho64(sys_, y, free):
    from phoenix_amd.simulator import rates_reference
    return np.where(free, np.abs(rates_reference(sys_, y.astype(np.float64))), 0).max(axis=1)


def floor32(sys_, y, free):
    """r32 [B]: the largest difference between the float32 and the float64 interpretation of the rates at y"""
    from phoenix_amd.simulator import rates_reference
    d = rates_reference(sys_, y, dtype=np.float32).astype(np.float64) - rates_reference(sys_, y.astype(np.float64))
    return np.where(free, np.abs(d), 0).max(axis=1)


def kappa(sys_, y_ref, free):
    """[B]: the infinity norm of the inverse of the float64 Jacobian on the moving genes at y_ref"""
    J = dense_jacobian(sys_, y_ref)
    return np.array([np.abs(np.linalg.inv(J[b][np.ix_(free[b], free[b])])).sum(axis=1).max() if free[b].any() else 0.0
                     for b in range(len(free))])


def check(sys_, x0, free, y_ref, got, what, tol=TOL, slack=None):
    """status 0; residual64 <= tol + r32; distance <= 2 kappa (tol + r32 + slack); genes that do not move keep x0's bits"""
    B = len(x0)
    y = got.y.cpu().numpy()
    assert got.status.tolist() == [0] * B, got.status.tolist()
    assert got.y.dtype == torch.float32 and got.iterations.dtype == torch.int32 and got.status.dtype == torch.int32
    assert got.reduced is None and got.y.shape == x0.shape and got.tau.shape == (B,)
    r32, kap = floor32(sys_, y, free), kappa(sys_, y_ref, free)
    res, dist = rho64(sys_, y, free), np.abs(y - y_ref).max(axis=1)
    bound = 2 * kap * (tol + r32 + (0 if slack is None else slack))
    live = bound > 0
    print("%s: steps %s, residual64 / (tol + r32) %.3f, distance / bound %.3f, kappa up to %.1f, r32 up to %.1e"
          % (what, got.iterations.tolist(), (res / (tol + r32)).max(), (dist[live] / bound[live]).max() if live.any() else 0.0,
             kap.max(), r32.max()))
    assert np.all(res <= tol + r32), (res, r32)
    assert np.all(dist <= bound), (dist, bound)
    assert np.array_equal(y[~free], x0[~free])
    assert np.all(got.residual.cpu().numpy() <= tol) and np.all(got.iterations.cpu().numpy() <= 50)
    return r32, kap


@pytest.mark.parametrize("method", ["blocks", "dense"])
@pytest.mark.parametrize("name", CASES)
def test_steady_states_against_the_reference(dev, name, method):
    sys_, x0, clamp, frozen = case(name)
    ref = reference(name)
    assert np.all(ref.status == 0)
    dsys, tx0 = on_device(name, dev)
    fz = None if frozen is None else torch.from_numpy(frozen).to(dev)
    got = dsys.steady_states(tx0, clamp=clamp, frozen=fz, tol=TOL, method=method)
    check(sys_, x0, moving(name), ref.y, got, "%s, %s" % (name, method))
    if method == "blocks":
        auto = dsys.steady_states(tx0, clamp=clamp, frozen=fz, tol=TOL)
        assert all(torch.equal(a, b) for a, b in zip(auto[:5], got[:5]))           # None picks the kernel below the cap


def test_a_component_above_the_cap_takes_the_dense_route(dev):
    from phoenix_amd.simulator import HillSystem, steady_states_reference
    N, B = 350, 6
    names, exprs, info = synthetic_network(N)
    sys_ = HillSystem(names, exprs, device="cpu")
    assert sys_.block_structure().largest > 64
    x0 = synthetic_states(N, B, info)
    ref = steady_states_reference(sys_, x0, tol=1e-12, max_iter=40)
    assert np.all(ref.status == 0)
    dsys = HillSystem(names, exprs, device=dev)
    with pytest.raises(ValueError, match="largest component"):
        dsys.steady_states(torch.from_numpy(x0).to(dev), method="blocks")
    got = dsys.steady_states(torch.from_numpy(x0).to(dev), tol=TOL)
    check(sys_, x0, np.repeat(~sys_.is_input[None], B, axis=0), ref.y, got, "synthetic 350, None -> dense")
    dense = dsys.steady_states(torch.from_numpy(x0).to(dev), tol=TOL, method="dense")
    assert torch.equal(dense.y, got.y)


@pytest.mark.parametrize("name", CASES)
def test_a_rows_bits_do_not_depend_on_the_batch(dev, name):
    _, _, clamp, frozen = case(name)
    dsys, tx0 = on_device(name, dev)
    B = tx0.shape[0]
    clamp = [()] * B if clamp is None else clamp
    free = torch.from_numpy(moving(name)).to(dev)
    kw = dict(tol=TOL, method="blocks")
    full = dsys.steady_states(tx0, clamp=clamp, frozen=~free, **kw)                 # frozen [B, N] says the same again
    plain = dsys.steady_states(tx0, clamp=clamp, frozen=None if frozen is None else torch.from_numpy(frozen).to(dev), **kw)
    rev = dsys.steady_states(tx0.flip(0).contiguous(), clamp=clamp[::-1], frozen=(~free).flip(0), **kw)
    twice = dsys.steady_states(tx0.repeat(2, 1), clamp=clamp + clamp, frozen=(~free).repeat(2, 1), **kw)
    for f in range(5):
        assert torch.equal(full[f], plain[f]) and torch.equal(full[f], rev[f].flip(0))
        assert torch.equal(full[f], twice[f][:B]) and torch.equal(full[f], twice[f][B:])
    for b in (0, 1, B - 1):
        one = dsys.steady_states(tx0[b:b + 1], clamp=clamp[b:b + 1], frozen=~free[b:b + 1], **kw)
        for f in range(5):
            assert torch.equal(full[f][b:b + 1], one[f]), (b, f)
    again = dsys.steady_states(tx0.unsqueeze(1), clamp=clamp, frozen=~free, **kw)      # [B, 1, N]
    assert torch.equal(again.y, full.y)


def test_control(dev):
    from phoenix_amd.simulator import HillSystem
    sys_, x0, clamp, _ = case("syn40")
    dsys, tx0 = on_device("syn40", dev)
    free = moving("syn40")
    full = dsys.steady_states(tx0, clamp=clamp, tol=TOL, method="blocks")
    its = full.iterations.cpu().numpy()
    assert its.min() >= 2
    for method in ("blocks", "dense"):
        # max_iter = 0: x0, with the status that rho decides
        none = dsys.steady_states(tx0, clamp=clamp, tol=TOL, max_iter=0, method=method)
        assert torch.equal(none.y, tx0) and none.y.data_ptr() != tx0.data_ptr()
        assert none.status.tolist() == [1] * 6 and none.iterations.tolist() == [0] * 6
        assert torch.equal(none.residual, torch.where(torch.from_numpy(free).to(dev), dsys.rhs(tx0).abs(), 0.0).amax(dim=1))
        done = dsys.steady_states(full.y, clamp=clamp, tol=TOL, max_iter=0, method=method)
        assert done.status.tolist() == [0] * 6 and torch.equal(done.y, full.y)
        two = dsys.steady_states(tx0, clamp=clamp, tol=TOL, max_iter=1, method=method)
        assert two.iterations.tolist() == [1] * 6
        accepted = (two.tau > 1.0).cpu().numpy()               # tau0 = 1 grows on an accepted step and shrinks on a refused one
        assert np.array_equal(two.y.cpu().numpy()[~accepted], x0[~accepted])
    # a row that converges at step k has the same bits under any larger max_iter
    for k in sorted(set([int(its.min()), int(its.max()), int(its.max()) + 9])):
        part = dsys.steady_states(tx0, clamp=clamp, tol=TOL, max_iter=k, method="blocks")
        done = torch.from_numpy(its <= k).to(dev)
        assert part.status.tolist() == np.where(its <= k, 0, 1).tolist()
        assert torch.equal(part.y[done], full.y[done]) and torch.equal(part.iterations[done], full.iterations[done])
        assert np.all(part.iterations.cpu().numpy()[its > k] == k)
    # Newton on a regulated gene without decay: sigma - J_AA = 0 ends the row with status 2, without a fault
    flat = HillSystem(["B", "A"], ["input gene", "((0.9 * fAct(B, 0.3, 2)) * 1 - 0 * A) / 1"], device=dev)
    x = torch.tensor([[0.6, 0.2], [0.0, 0.2]], device=dev)                  # (the second row is at rest: fAct(0) = 0)
    for method in ("blocks", "dense"):
        r = flat.steady_states(x, tau0=float("inf"), method=method)
        assert r.status.tolist() == [2, 0] and r.iterations.tolist() == [1, 0] and torch.equal(r.y, x), method


def test_knockout_steady_states(dev):
    from phoenix_amd.simulator import steady_states_reference
    name = "syn40"
    sys_, x0, _, _ = case(name)
    info = synthetic_network(40)[2]
    dsys, tx0 = on_device(name, dev)
    N, B = sys_.N, len(x0)
    g = gene_with_descendants(sys_, info)
    lone = next(j for j in range(N) if not descendants(sys_, j).any())
    genes, values = [g, lone, g], [0.0, 0.9, 1.3]
    K = len(genes)
    res = dsys.knockout_steady_states(tx0, genes, value=values, tol=TOL)
    base = dsys.steady_states(tx0, tol=TOL)
    assert res.genes == genes and res.shift.shape == (K, N) and res.knockouts.y.shape == (K * B, N)
    assert base.status.tolist() == [0] * B and res.knockouts.status.tolist() == [0] * (K * B)
    for a, b in zip(res.base[:5], base[:5]):
        assert torch.equal(a, b)
    d = res.knockouts.y.reshape(K, B, N) - base.y.unsqueeze(0)
    assert torch.equal(res.shift, d.mean(dim=1)) and torch.equal(res.magnitude, d.abs().mean(dim=1))
    shift, mag = res.shift.cpu().numpy(), res.magnitude.cpu().numpy()
    by = base.y.cpu().numpy()
    ky = res.knockouts.y.reshape(K, B, N).cpu().numpy()
    for k in range(K):
        reach = descendants(sys_, genes[k])
        still = ~reach
        still[genes[k]] = False
        assert not shift[k][still].any() and not mag[k][still].any()                # exactly 0 where the gene does not reach
        assert np.array_equal(ky[k][:, still], by[:, still])                        # ... the baseline's bits
        assert np.all(ky[k][:, genes[k]] == np.float32(values[k]))
        # the rest against the float64 fixed point from the same start, under the derived bound
        start = by.copy()
        start[:, genes[k]] = np.float32(values[k])
        free = np.repeat((reach & ~sys_.is_input)[None], B, axis=0)
        free[:, genes[k]] = False
        ref = steady_states_reference(sys_, start, clamp=[(genes[k],)] * B, frozen=~free[0], tol=1e-12, max_iter=40)
        assert np.all(ref.status == 0)
        got = type(base)(*(x[k * B:(k + 1) * B] for x in res.knockouts[:5]), None)
        check(sys_, start, free, ref.y, got, "knockout of gene %d at %.1f" % (genes[k], values[k]))
    assert res.knockouts.iterations.reshape(K, B)[1].tolist() == [0] * B            # nothing to move: done at once
    assert np.abs(np.delete(shift[0], genes[0])).max() > 1e-4                       # a knockout that does reach its targets
    # whatever the block size and the route
    for kw in (dict(rows_per_call=4), dict(rows_per_call=7)):
        other = dsys.knockout_steady_states(tx0, genes, value=values, tol=TOL, **kw)
        assert torch.equal(other.knockouts.y, res.knockouts.y) and torch.equal(other.shift, res.shift)
    dense = dsys.knockout_steady_states(tx0, genes, value=values, tol=TOL, method="dense")
    for k in range(K):
        still = ~descendants(sys_, genes[k])
        still[genes[k]] = False
        assert not dense.shift.cpu().numpy()[k][still].any()
    assert dense.knockouts.status.tolist() == [0] * (K * B)


def test_against_the_integrator(dev):
    """`simulate` to T = 30 at dt_max = 0.01 ends within 2 kappa (rho64(x(T)) + tol + r32) of the kernel's state on g11"""
    sys_, x0, _, _ = case("g11")
    dsys, tx0 = on_device("g11", dev)
    free = moving("g11")
    got = dsys.steady_states(tx0, tol=TOL, method="blocks")
    r32, kap = check(sys_, x0, free, reference("g11").y, got, "g11")
    xT = dsys.simulate(tx0, [0.0, 30.0], dt_max=0.01)[-1].cpu().numpy()
    rT = rho64(sys_, xT, free)
    dist = np.abs(xT - got.y.cpu().numpy()).max(axis=1)
    print("rho64(x(30)) up to %.1e, |x(30) - steady state| / bound %.3f" % (rT.max(), (dist / (2 * kap * (rT + TOL + r32))).max()))
    assert np.all(dist <= 2 * kap * (rT + TOL + r32))


def test_steady_state_recovery(dev):
    import phoenix_amd
    from phoenix_amd.analysis import steady_state_recovery
    from test_gpu_parity import make_net
    from test_steady_cpu import make_model
    sys_, x0, _, _ = case("syn96")
    info = synthetic_network(96)[2]
    dsys, _ = on_device("syn96", dev)
    tx0 = torch.from_numpy(np.clip(x0, 0.0, 1.0)).to(dev)
    net = make_net(phoenix_amd, dev, make_model(96, 44, 5)[0])       # a model whose steady states tests/test_steady_gpu.py solves
    genes = [g for g in range(96) if not info["is_input"][g] and descendants(sys_, g).any()][:4]
    r = steady_state_recovery(net, dsys, tx0, genes, value=0.0, tol=TOL)
    assert r.genes == genes and r.true.shift.shape == r.learned.shift.shape == (4, 96)
    assert 0 <= r.n_unconverged <= 5 * 6 and r.n_entries > 0
    counted = r.per_gene.n_entries.sum()
    assert counted == r.n_entries
    if r.n_unconverged == 0:
        want = phoenix_amd.knockout_recovery_scores(genes, r.true.shift, r.learned.shift)
        assert want.n_entries == r.n_entries and np.isclose(want.pearson, r.pearson, rtol=1e-5, atol=1e-7)
    for v in (r.sign_agreement, r.pearson, r.spearman, r.slope, r.base_pearson, r.base_rms):
        assert np.isfinite(v), r[:11]
