"""GPU tests of the steady-state solve: the MFMA kernel phx_reduced_jacobian against its float64 formulas under a derived
bound, its bits under regrouping of the states, `steady_states` against `steady_states_reference` and against the dopri5
solver the project already has, the per-row control, and `knockout_steady_states`.  Models and float64 formulas:
tests/test_steady_cpu.py, whose reference results (all rows converged) these comparisons rest on."""
import numpy as np
import pytest
import torch

from test_gpu_parity import make_net
from test_steady_cpu import SHAPES, C64, dense_jacobian, make_model, moving, parts64, reference, rho64

pytestmark = pytest.mark.gpu
U = 2.0 ** -24
TOL = 1e-5


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "these tests need the MI355X"
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def pa():
    import phoenix_amd
    return phoenix_amd


def params_of_net(pa, net):
    from phoenix_amd import engine
    from phoenix_amd.odenet import params_of
    return engine.params_cached(*params_of(net))


def kernel_inputs(N, H, B):
    """(p, y, m, r) float32: m from [0, 1] with exact zeros (a third of the genes, and all of the last state when B >= 2)"""
    p, y0, _ = make_model(N, H, B)
    rng = np.random.default_rng(1000 + N)
    m = rng.random((B, N)).astype(np.float32)
    m[rng.random((B, N)) < 0.33] = 0.0
    m[0, 0] = 1.0
    if B >= 2:
        m[B - 1] = 0.0
    r = (0.1 * rng.standard_normal((B, N))).astype(np.float32)
    return p, y0, m, r


def kernel_truth(p, y, m, r):
    """float64 on the same float32 inputs: (S, w, hid) and the same formulas on absolute values (AS, Aw, Ahid), with the
    relative error bound rel_v [B, H] of v = exp(Wp l + bp) computed in float32"""
    B, N = y.shape
    H = p["Ws"].shape[0]
    q = {k: v.astype(np.float64) for k, v in p.items()}
    a, l, da, dl, hid, _ = parts64(p, y)
    m, r = m.astype(np.float64), r.astype(np.float64)
    k = (N + 18) * U / (1 - (N + 18) * U)
    Ez = k * (np.abs(l) @ np.abs(q["Wp"]).T + np.abs(q["bp"]))             # error of the exponent
    rel_v = np.expm1(Ez) + 4 * U
    S, w, AS, Aw = (np.empty(s) for s in ((B, 2 * H, 2 * H), (B, 2 * H), (B, 2 * H, 2 * H), (B, 2 * H)))
    for b in range(B):
        Cm = np.concatenate([q["Ws"] * (da[b] * m[b])[None, :], hid[b, H:, None] * q["Wp"] * (dl[b] * m[b])[None, :]], axis=0)
        S[b], w[b] = Cm @ q["Wa"], Cm @ r[b]
        AS[b], Aw[b] = np.abs(Cm) @ np.abs(q["Wa"]), np.abs(Cm) @ np.abs(r[b])
    Ahid = np.concatenate([np.abs(a) @ np.abs(q["Ws"]).T + np.abs(q["bs"]), hid[:, H:]], axis=1)
    return S, w, hid, AS, Aw, Ahid, rel_v, k


@pytest.mark.parametrize("N,H,B", SHAPES)
@pytest.mark.parametrize("with_r", [True, False])
def test_kernel_against_float64(pa, dev, N, H, B, with_r):
    """The bar, derived.  An entry of S, w or of the sums half of hid is a float32 dot product of N terms, summed in the
    kernel's order (fmaf chains of the MFMA, lanes, segments): for any order |fl(sum) - sum| <= gamma_N sum |terms|.  A term
    carries a fixed count of roundings besides: at most 16 in a, l, a', l' for y in [0, 1) (correctly rounded + - * /, log1pf to
    2 ulp at a condition number <= 1.5) and 2 in the scalings by m and by r.  So with k = (N + 18) u / (1 - (N + 18) u),
    u = 2^-24, and A the same formula on absolute values:   |got - ref64| <= k A   for the sums rows.
    A product row is v_j times such a contraction; v_j = exp(z_j), z_j an N-term float32 contraction with
    |z_j - z64_j| <= E_j = k (sum |Wp| |l| + |bp|), so v_j has the relative error rel_j = expm1(E_j) + 4 u (expf to 2 ulp, the
    rounding of the product, and slack), and   |got - ref64| <= (k (1 + rel_j) + rel_j) v_j A   for the product rows of S
    and w, rel_j v_j for those of hid.  Where A is 0 the result is exactly 0."""
    from phoenix_amd import engine
    p, y, m, r = kernel_inputs(N, H, B)
    net = make_net(pa, dev, p)
    P = params_of_net(pa, net)
    t = lambda x: torch.from_numpy(x).to(dev)      # noqa: E731
    S, w, hid = engine.reduced_jacobian(P, t(y), t(m), t(r) if with_r else None)
    assert (w is None) == (not with_r) and S.shape == (B, 2 * H, 2 * H) and hid.shape == (B, 2 * H) and S.dtype == torch.float32
    S64, w64, hid64, AS, Aw, Ahid, rel_v, k = kernel_truth(p, y, m, r)
    rel = np.concatenate([np.zeros((B, H)), rel_v], axis=1)                 # per row j of the 2H
    bar_S = (k * (1 + rel) + rel)[:, :, None] * AS
    bar_w = (k * (1 + rel) + rel) * Aw
    bar_hid = np.where(np.arange(2 * H)[None, :] < H, k * Ahid, rel * Ahid)
    worst = {}
    for name, got, ref, bar, A in (("S", S, S64, bar_S, AS), ("hid", hid, hid64, bar_hid, Ahid)) + \
            ((("w", w, w64, bar_w, Aw),) if with_r else ()):
        got = got.cpu().numpy().astype(np.float64)
        assert np.all(np.isfinite(got)), name
        assert np.all(got[A == 0] == 0), name
        err = np.abs(got - ref)
        worst[name] = float((err[A > 0] / bar[A > 0]).max())
    if B >= 2:
        assert not S[B - 1].any() and (not with_r or not w[B - 1].any())       # the state of weight 0: exact zeros
    print("(%d, %d, %d) r=%s: worst error / bar %s" % (N, H, B, with_r, {n: "%.3f" % v for n, v in worst.items()}))
    for name, v in worst.items():
        assert v <= 1.0, (name, v)


@pytest.mark.parametrize("N,H,B", [(97, 7, 5), (130, 40, 3), (161, 200, 2), (513, 97, 6), (1100, 48, 6)])
def test_a_states_bits_do_not_depend_on_the_call(pa, dev, N, H, B):
    from phoenix_amd import engine
    p, y, m, r = kernel_inputs(N, H, B)
    P = params_of_net(pa, make_net(pa, dev, p))
    y, m, r = (torch.from_numpy(x).to(dev) for x in (y, m, r))
    full = engine.reduced_jacobian(P, y, m, r)
    again = engine.reduced_jacobian(P, y, m, r)
    for a, b in zip(full, again):
        assert torch.equal(a, b)
    rev = engine.reduced_jacobian(P, y.flip(0).contiguous(), m.flip(0).contiguous(), r.flip(0).contiguous())
    twice = engine.reduced_jacobian(P, y.repeat(2, 1), m.repeat(2, 1), r.repeat(2, 1))
    for a, b, c in zip(full, rev, twice):
        assert torch.equal(a, b.flip(0)) and torch.equal(a, c[:B]) and torch.equal(a, c[B:])
    for b in range(B):
        one = engine.reduced_jacobian(P, y[b:b + 1], m[b:b + 1], r[b:b + 1])
        for a, o in zip(full, one):
            assert torch.equal(a[b:b + 1], o), b
    # the passes of the iteration likewise: the residual, the solve and the update of a row alone
    hid, res = engine.steady_residual(P, y)
    x, info = engine.steady_solve(full[0], full[1])
    up = engine.steady_update(P, y, m, r, x)
    for b in (0, B - 1):
        h1, r1 = engine.steady_residual(P, y[b:b + 1])
        x1, i1 = engine.steady_solve(full[0][b:b + 1].contiguous(), full[1][b:b + 1].contiguous())
        u1 = engine.steady_update(P, y[b:b + 1], m[b:b + 1], r[b:b + 1], x1)
        assert torch.equal(h1, hid[b:b + 1]) and torch.equal(r1, res[b:b + 1]) and torch.equal(x1, x[b:b + 1])
        assert torch.equal(u1, up[b:b + 1]) and int(i1) == int(info[b]) == 0
    assert torch.equal(up[m == 0], y[m == 0])


def test_the_passes_of_the_iteration_against_float64(pa, dev):
    """the residual, the dense solve and the update against numpy float64 on the same inputs (bounds as above: N- and 2H-term
    float32 contractions; the solve is float64 inside and rounds its result once)"""
    from phoenix_amd import engine
    for N, H, B in ((97, 7, 5), (200, 200, 2), (513, 97, 2)):
        p, y, m, r = kernel_inputs(N, H, B)
        P = params_of_net(pa, make_net(pa, dev, p))
        ty, tm, tr = (torch.from_numpy(x).to(dev) for x in (y, m, r))
        S, w, hid = engine.reduced_jacobian(P, ty, tm, tr)
        hid2, res = engine.steady_residual(P, ty)
        _, _, _, _, hid64, r64 = parts64(p, y)
        k = (N + 18) * U / (1 - (N + 18) * U)
        q = {key: v.astype(np.float64) for key, v in p.items()}
        hd = hid2.cpu().numpy().astype(np.float64)             # the residual is formed from the pass's own hidden vector
        bar_r = (2 * H + 2) * U * (np.abs(hd) @ np.abs(q["Wa"]).T + np.abs(y)) + np.abs(hd - hid64) @ np.abs(q["Wa"]).T
        assert np.all(np.abs(res.cpu().numpy() - r64) <= bar_r)
        Ahid, rel_v = kernel_truth(p, y, m, r)[5:7]
        bar_hid = np.concatenate([k * Ahid[:, :H], rel_v * Ahid[:, H:]], axis=1)          # the bars of the kernel's hid
        assert np.all(np.abs(hid2.cpu().numpy() - hid64) <= bar_hid)
        x, info = engine.steady_solve(S, w)
        assert not info.any()
        S_, w_ = S.cpu().numpy().astype(np.float64), w.cpu().numpy().astype(np.float64)
        x64 = np.stack([np.linalg.solve(np.eye(2 * H) - S_[b], w_[b]) for b in range(B)])
        cond = max(np.linalg.cond(np.eye(2 * H) - S_[b]) for b in range(B))
        assert np.abs(x.cpu().numpy() - x64).max() <= (U + 1e-13 * cond) * max(1.0, np.abs(x64).max())
        up = engine.steady_update(P, ty, tm, tr, x).cpu().numpy()
        xs = x.cpu().numpy().astype(np.float64)
        z = xs @ q["Wa"].T
        want = y + m.astype(np.float64) * (r + z)
        bar = (2 * H + 4) * U * (np.abs(y) + m * (np.abs(r) + np.abs(xs) @ np.abs(q["Wa"]).T))
        assert np.all(np.abs(up - want) <= bar) and np.array_equal(up[m == 0], y[m == 0])
    # a singular and a non-finite I - S are reported per state, and the healthy state beside them is solved
    S = torch.zeros((3, 4, 4), device=dev)
    S[0] = torch.eye(4)
    S[1, 2, 1] = float("nan")
    S[2] = 0.5 * torch.eye(4)
    x, info = engine.steady_solve(S, torch.ones((3, 4), device=dev))
    assert info.tolist()[0] > 0 and info.tolist()[1] != 0 and info.tolist()[2] == 0
    assert torch.equal(x[2], torch.full((4,), 2.0, device=dev)) and not x[:2].any()


_GPU = {}


def solved(pa, dev, N, H, B):
    """(net, steady_states at the default control) of a test shape, solved once per session"""
    if (N, H, B) not in _GPU:
        p, y0, held, _ = reference(N, H, B)
        net = make_net(pa, dev, p)
        _GPU[(N, H, B)] = (net, pa.steady_states(net, torch.from_numpy(y0).to(dev), clamp=held, tol=TOL))
    return _GPU[(N, H, B)]


def floor32(p, y_ref, free):
    """r32 [B]: the residual numpy's float32 arithmetic leaves at the reference's fixed point"""
    y = y_ref.astype(np.float32)
    s = y - np.float32(0.5)
    a = s / (1 + np.abs(s))
    l = np.log1p(a)
    hid = np.concatenate([a @ p["Ws"].T + p["bs"], np.exp(l @ p["Wp"].T + p["bp"])], axis=1)
    return np.where(free, np.abs(hid @ p["Wa"].T - y), 0).max(axis=1).astype(np.float64)


def kappa(p, y_ref, free):
    """[B]: the infinity norm of the inverse of the dense float64 I - diag(free) Wa C diag(free) at y_ref"""
    return np.array([np.abs(np.linalg.inv(dense_jacobian(p, y_ref, b, free[b]))).sum(axis=1).max() for b in range(len(free))])


def check_against_reference(p, y0, held, ref, got, tol=TOL):
    """status 0 everywhere; the float64 residual of the returned y <= tol + r32; |y - y_ref| <= 2 kappa (tol + r32); the
    genes that do not move equal y0 to the bit.  Both bounds come from the reference."""
    B = len(y0)
    free = moving(p, held, B)
    y = got.y.cpu().numpy()
    assert got.status.tolist() == [0] * B, got.status.tolist()
    assert got.y.dtype == torch.float32 and got.iterations.dtype == torch.int32 and got.status.dtype == torch.int32
    r32, kap = floor32(p, ref.y, free), kappa(p, ref.y, free)
    res = rho64(p, y, free)
    dist = np.abs(y - ref.y).max(axis=1)
    print("steps %s (reference %s), residual64 / (tol + r32) %.3f, distance / bound %.3f, kappa up to %.1f, r32 up to %.1e"
          % (got.iterations.tolist(), ref.iterations.tolist(), (res / (tol + r32)).max(), (dist / (2 * kap * (tol + r32))).max(),
             kap.max(), r32.max()))
    assert np.all(res <= tol + r32), (res, r32)
    assert np.all(dist <= 2 * kap * (tol + r32)), (dist, kap, r32)
    assert np.array_equal(y[~free], y0[~free])
    assert np.all(got.residual.cpu().numpy() <= tol) and np.all(got.iterations.cpu().numpy() <= 50)
    return r32, kap


@pytest.mark.parametrize("N,H,B", SHAPES)
def test_steady_states_against_the_reference(pa, dev, N, H, B):
    p, y0, held, ref = reference(N, H, B)
    assert np.all(ref.status == 0)
    net, got = solved(pa, dev, N, H, B)
    before = [x.detach().clone() for x in net.parameters()]
    check_against_reference(p, y0, held, ref, got)
    assert all(torch.equal(a, b) for a, b in zip(before, net.parameters()))           # the module is never modified
    assert got.reduced is None and got.y.shape == (B, N) and got.tau.shape == (B,)


def test_against_the_dopri5_solver(pa, dev):
    """odeint to T = 60 ends within 2 kappa (rho64(y(T)) + tol + r32) of the steady state, with rho64(y(T)) <= 1e-3"""
    N, H, B = 350, 30, 7
    p, y0, held = make_model(N, H, B, g_lo=0.5, g_hi=1.5)
    ref = pa.steady_states_reference(p, y0, clamp=held, tol=1e-12, max_iter=40)
    assert np.all(ref.status == 0)
    net = make_net(pa, dev, p)
    ty0 = torch.from_numpy(y0).to(dev)
    got = pa.steady_states(net, ty0, clamp=held, tol=TOL)
    r32, kap = check_against_reference(p, y0, held, ref, got)
    with torch.no_grad():
        yT = pa.odeint(net, ty0, torch.tensor([0.0, 60.0], dtype=torch.float64, device=dev), clamp=held,
                       options={"batch_control": "per_trajectory"})[-1].cpu().numpy()
    free = moving(p, held, B)
    rT = rho64(p, yT, free)
    dist = np.abs(yT - got.y.cpu().numpy()).max(axis=1)
    print("rho64(y(60)) %s, |y(60) - steady state| / bound %.3f" % (rT, (dist / (2 * kap * (rT + TOL + r32))).max()))
    assert np.all(rT <= 1e-3)
    assert np.all(dist <= 2 * kap * (rT + TOL + r32))


def test_control(pa, dev):
    from phoenix_amd import engine
    N, H, B = 350, 30, 7
    p, y0, held, ref = reference(N, H, B)
    net, full = solved(pa, dev, N, H, B)
    ty0 = torch.from_numpy(y0).to(dev)
    its = full.iterations.cpu().numpy()
    assert its.min() >= 3
    # max_iter = 2: status 1, two steps, and a state whose residual is the one reported -- the last accepted one
    two = pa.steady_states(net, ty0, clamp=held, tol=TOL, max_iter=2)
    assert two.status.tolist() == [1] * B and two.iterations.tolist() == [2] * B
    P = params_of_net(pa, net)
    free = torch.from_numpy(moving(p, held, B)).to(dev)
    rho = torch.where(free, engine.steady_residual(P, two.y)[1].abs(), torch.zeros((), device=dev)).amax(dim=1)
    assert torch.equal(rho, two.residual)
    one = pa.steady_states(net, ty0, clamp=held, tol=TOL, max_iter=1)
    accepted = (one.tau > 1.0).cpu().numpy()                   # tau0 = 1 grows on an accepted step and shrinks on a refused one
    assert np.array_equal(one.y.cpu().numpy()[~accepted], y0[~accepted])
    # a row that converges at step k has the same bits under any larger max_iter
    for k in sorted(set([int(its.min()), int(its.max()), int(its.max()) + 9])):
        part = pa.steady_states(net, ty0, clamp=held, tol=TOL, max_iter=k)
        done = its <= k
        assert part.status.cpu().numpy().tolist() == np.where(done, 0, 1).tolist()
        assert torch.equal(part.y[torch.from_numpy(done).to(dev)], full.y[torch.from_numpy(done).to(dev)])
        assert np.array_equal(part.iterations.cpu().numpy()[done], its[done]) and np.all(part.iterations.cpu().numpy()[~done] == k)
    # return_reduced: S with unit weights on the moving genes at the result
    red = pa.steady_states(net, ty0, clamp=held, tol=TOL, return_reduced=True)
    assert torch.equal(red.y, full.y)
    assert torch.equal(red.reduced, pa.reduced_jacobian(net, full.y, clamp=held))
    assert torch.equal(red.reduced, engine.reduced_jacobian(P, full.y, free.to(torch.float32))[0])
    assert np.abs(red.reduced.cpu().numpy() - ref.reduced).max() <= 1e-3
    half = pa.reduced_jacobian(net, full.y, weight=torch.full((N,), 0.5, device=dev), clamp=held)
    assert torch.equal(half, 0.5 * red.reduced)                # a power of two scales every term exactly


def test_plain_newton_on_the_weakest_model(pa, dev):
    """tau0 = inf is Newton's iteration from the first step; on the weakest test model it converges, to the fixed point of
    the reference run the same way"""
    N, H, B = NEWTON_SHAPE
    p, y0, held, _ = reference(N, H, B)
    ref = pa.steady_states_reference(p, y0, clamp=held, tol=1e-12, max_iter=40, tau0=float("inf"))
    assert np.all(ref.status == 0)
    net, _ = solved(pa, dev, N, H, B)
    got = pa.steady_states(net, torch.from_numpy(y0).to(dev), clamp=held, tol=TOL, tau0=float("inf"))
    check_against_reference(p, y0, held, ref, got)
    assert torch.isinf(got.tau).all() and np.all(got.iterations.cpu().numpy() <= 40)


NEWTON_SHAPE = (200, 200, 2)                   # spectral radius of S at the fixed points 0.36: the weakest coupling of the shapes


def test_knockout_steady_states(pa, dev):
    N, H, B = 96, 44, 5
    p, y0, _ = make_model(N, H, B)
    p = {k: v.copy() for k, v in p.items()}
    quiet, deaf = 11, [20, 21, 22]             # a gene that regulates nobody, and genes that nobody regulates
    assert p["g"][quiet] > 0 and np.all(p["g"][deaf] > 0)
    p["Ws"][:, quiet] = 0
    p["Wp"][:, quiet] = 0
    p["Wa"][deaf, :] = 0                       # their residual is -y: at 0 they stay, to the bit
    y0 = y0.copy()
    y0[:, deaf] = 0
    net = make_net(pa, dev, p)
    ty0 = torch.from_numpy(y0).to(dev)
    genes, values = [5, quiet, 40], [0.0, 0.9, 0.0]
    res = pa.knockout_steady_states(net, ty0, genes, value=values, tol=TOL)
    K = len(genes)
    base = pa.steady_states(net, ty0, tol=TOL)
    assert base.status.tolist() == [0] * B and res.knockouts.status.tolist() == [0] * (K * B)
    for a, b in zip(res.base[:5], base[:5]):
        assert torch.equal(a, b)
    # the calls it stands for, bit for bit, whatever the block size
    start = base.y.unsqueeze(0).repeat(K, 1, 1)
    for k in range(K):
        start[k, :, genes[k]] = values[k]
    clamp = [(g,) for g in genes for _ in range(B)]
    direct = pa.steady_states(net, start.reshape(K * B, N), clamp=clamp, tol=TOL)
    others = [pa.knockout_steady_states(net, ty0, genes, value=values, tol=TOL, rows_per_call=n) for n in (4, 7)]
    rows = [pa.steady_states(net, start.reshape(K * B, N)[i:i + 1], clamp=clamp[i:i + 1], tol=TOL) for i in (0, 7, 14)]
    for f in range(5):
        assert torch.equal(res.knockouts[f], direct[f])
        for o in others:
            assert torch.equal(res.knockouts[f], o.knockouts[f]) and torch.equal(res.shift, o.shift)
        for i, one in zip((0, 7, 14), rows):
            assert torch.equal(res.knockouts[f][i:i + 1], one[f])
    d = res.knockouts.y.reshape(K, B, N) - base.y.unsqueeze(0)
    assert torch.equal(res.shift, d.mean(dim=1)) and torch.equal(res.magnitude, d.abs().mean(dim=1))
    assert res.shift.shape == (K, N) and res.genes == genes
    shift = res.shift.cpu().numpy()
    # the held gene sits at its level; a gene that regulates nobody moves nobody, and its rows are done at once
    for k in range(K):
        assert np.all(res.knockouts.y.reshape(K, B, N)[k, :, genes[k]].cpu().numpy() == np.float32(values[k]))
    assert not np.delete(shift[1], quiet).any() and not np.delete(res.magnitude.cpu().numpy()[1], quiet).any()
    assert res.knockouts.iterations.reshape(K, B)[1].tolist() == [0] * B
    # genes that nobody regulates cannot be reached by any held gene: exactly 0
    assert not shift[:, deaf].any() and not base.y[:, deaf].any()
    assert np.abs(np.delete(shift[0], genes[0])).max() > 1e-4          # a knockout that does reach its targets
    names, scores = pa.consolidate_gene_scores(["g%d" % n for n in range(N)], res.magnitude[0])     # a per-gene vector
    assert len(names) == N == len(scores)
