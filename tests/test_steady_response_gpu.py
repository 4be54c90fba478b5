"""GPU tests of the total-effects network at a fixed point: each stage of phx_steady_resp.hip at the C
boundary against float64 on the same float32 inputs under a derived componentwise bound, `steady_state_response` against
`steady_state_response_reference` at the float32 states of `steady_states` under the stages' bounds propagated to first
order, the bits of regulator blocks, the exact values, the rows that are left out, and the cross-check with the implicit
adjoint.  Models and float64 formulas: tests/test_steady_cpu.py; the bound of phx_reduced_jacobian: tests/test_steady_gpu.py."""
import numpy as np
import pytest
import scipy.linalg
import torch

from test_gpu_parity import make_net
from test_steady_adjoint_gpu import back64
from test_steady_cpu import make_model, moving, parts64, reference
from test_steady_gpu import kernel_truth
from test_steady_response_cpu import singular_model

pytestmark = pytest.mark.gpu
U = 2.0 ** -24
U64 = 2.0 ** -53
# (N, H, B): 2H no multiple of 4, the 16- and 64-wide edges, N no multiple of 64, the worst cond(I - S) of the test models
# (96, 56, 4), one, two and three states for the double buffer, both sides of 2H = 128 (the WaT panel stays in LDS up to
# there), and H = 256 for the LDS budget
SHAPES = [(33, 1, 1), (37, 5, 3), (97, 7, 5), (96, 56, 4), (130, 40, 3), (70, 97, 3), (161, 200, 1), (513, 97, 2), (70, 256, 2)]
INPUTS = ("level", "production")


def gamma(k, u=U):
    return k * u / (1 - k * u)


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "these tests need the MI355X"
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def pa():
    import phoenix_amd
    return phoenix_amd


def engine_params(net):
    from phoenix_amd import engine
    from phoenix_amd.odenet import params_of
    return engine.params_cached(*params_of(net))


def w64(p):
    return {k: v.astype(np.float64) for k, v in p.items()}


# --------------------------------------------------------------------------- float64 stages and their bounds
def reduced64(p, y, m):
    """S [B, 2H, 2H] float64 at the float32 states y with the weights m"""
    q = w64(p)
    H = q["Ws"].shape[0]
    _, _, da, dl, hid, _ = parts64(p, y)
    return np.stack([np.concatenate([q["Ws"] * (da[b] * m[b])[None, :], hid[b, H:, None] * q["Wp"] * (dl[b] * m[b])[None, :]], axis=0)
                     @ q["Wa"] for b in range(len(y))])


def inverse64(S, dS=None):
    """(Z, bar): Z_b = (I - S_b)^-1 in float64 and the bound of the device's float result.  The device forms I - S exactly in
    double (a float minus 1 is a double), factors it with partial pivoting -- |dA| <= gamma64_3n |L| |U| (Higham, Theorem 9.4),
    L and U from scipy's LU of the same matrix, the same pivot rule -- so a column of the inverse carries |Z| |dA| |Z| to
    first order (doubled for the higher orders), and the result is rounded to float once: u |Z|.  dS: a bound of an error of
    S itself, propagated the same way, |Z| dS |Z|."""
    n = S.shape[1]
    Z, bar = np.empty_like(S), np.empty_like(S)
    for b in range(len(S)):
        A = np.eye(n) - S[b]
        Z[b] = np.linalg.inv(A)
        _, L, Um = scipy.linalg.lu(A)
        E = gamma(3 * n, U64) * (np.abs(L) @ np.abs(Um))
        if dS is not None:
            E = E + dS[b]
        bar[b] = U * np.abs(Z[b]) + 2 * np.abs(Z[b]) @ E @ np.abs(Z[b])
    return Z, bar


def factors64(p, y, m, hid, Z, regs, input, dZ=None, rel_v=None):
    """(Xs [B, 2H, K], d [B, K], bar [B, 2H, K]) float64 from the inputs as they are given, and the bound of the device's X.
    The unscaled column: two H-term float32 contractions in any order, one rounding in Z v, at most 5 in a' and 7 in l'
    (correctly rounded + - * /), two in the products with them and one in their sum (an fma): k1 = H + 12 roundings,
    dX = gamma_k1 (a' |Zs| |Ws| + l' |Zp| v |Wp|).  d = 1 + m dot: a 2H-term chain on the device's own X and one fma:
    dd = m (gamma_(2H + 1) |Wa| (|X| + dX) + |Wa| dX) + u |d|.  Level: |x^ / d^ - x / d| <= dX / |d| + (|X| + dX) dd / (|d| (|d| -
    dd)) and the rounding of the division, u |x / d| (1 + ...): the bound below takes 2 u.  Production: the product with m
    (0 or 1) is exact.  dZ, rel_v: bounds of errors of Z and relative errors of v = hid[:, H:], propagated to first order
    (the term of d is then |X| dd / d^2)."""
    q = w64(p)
    H = q["Ws"].shape[0]
    B, K = len(y), len(regs)
    _, _, da, dl, _, _ = parts64(p, y)
    Xs, d, bar = np.empty((B, 2 * H, K)), np.empty((B, K)), np.empty((B, 2 * H, K))
    k1 = H + 12
    for b in range(B):
        Zs, Zp, v = Z[b][:, :H], Z[b][:, H:], hid[b, H:]
        ws, wp, a1, l1 = q["Ws"][:, regs], q["Wp"][:, regs], da[b, regs][None, :], dl[b, regs][None, :]
        X = a1 * (Zs @ ws) + l1 * ((Zp * v[None, :]) @ wp)
        AX = a1 * (np.abs(Zs) @ np.abs(ws)) + l1 * ((np.abs(Zp) * v[None, :]) @ np.abs(wp))
        dX = gamma(k1) * AX
        if dZ is not None:
            rv = np.zeros(H) if rel_v is None else rel_v[b]
            dX = dX + (1 + gamma(k1)) * (a1 * (dZ[b][:, :H] @ np.abs(ws)) +
                                         l1 * ((dZ[b][:, H:] * (v * (1 + rv))[None, :] + np.abs(Zp) * (v * rv)[None, :]) @ np.abs(wp)))
        wa = q["Wa"][regs]                                              # [K, 2H]
        mk = m[b, regs].astype(np.float64)
        dot = np.einsum("kc,ck->k", wa, X)
        d[b] = 1 + mk * dot
        dd = mk * (gamma(2 * H + 1) * np.einsum("kc,ck->k", np.abs(wa), np.abs(X) + dX) + np.einsum("kc,ck->k", np.abs(wa), dX)) \
            + U * np.abs(d[b])
        if input == "production":
            Xs[b], bar[b] = X * mk[None, :], dX * mk[None, :]
        else:
            Xs[b] = X / d[b][None, :]
            if dZ is None:
                assert np.all(np.abs(d[b]) > 2 * dd)
                over = (np.abs(X) + dX) * (dd / (np.abs(d[b]) * (np.abs(d[b]) - dd)))[None, :]
            else:                                                       # propagated errors: to first order, doubled by the caller
                over = np.abs(X) * (dd / d[b] ** 2)[None, :]
            bar[b] = dX / np.abs(d[b]) + over + 2 * U * np.abs(Xs[b])
    return Xs, d, bar


def response64(p, m, Xs, use, regs, input, mean_abs, dXs=None):
    """(out [K, N], bar) float64: the mean over the used states of m_bj sum_c Wa[j, c] Xs_b[c, k] (of its absolute value), the
    diagonal of the input.  Per state a 2H-term float32 chain, the product with m, the sum with m use on the production
    diagonal, then B - 1 additions and the division: k3 = 2H + B + 3 roundings times the same formula on absolute values;
    dXs: a bound of an error of Xs, propagated through |Wa| (the absolute value and the mean are non-expansive)."""
    q = w64(p)
    B, N, K = len(m), m.shape[1], len(regs)
    at = np.arange(K)
    acc, A, prop = np.zeros((K, N)), np.zeros((K, N)), np.zeros((K, N))
    for b in range(B):
        mb = m[b].astype(np.float64)
        T = (q["Wa"] @ Xs[b]).T * mb[None, :]                            # [K, N]
        AT = (np.abs(q["Wa"]) @ np.abs(Xs[b])).T * mb[None, :]
        if input == "production":
            T[at, regs] += mb[regs] * use[b]
            AT[at, regs] += mb[regs] * use[b]
        else:
            T[at, regs] = 0
            AT[at, regs] = 0
        acc += np.abs(T) if mean_abs else T
        A += AT
        if dXs is not None:
            P = (np.abs(q["Wa"]) @ dXs[b]).T * mb[None, :]
            if input == "level":
                P[at, regs] = 0
            prop += P
    cnt = use.sum(axis=0)
    div = np.where(cnt > 0, cnt, 1)[:, None]
    out, A, prop = acc / div, A / div, prop / div
    k3 = Xs.shape[1] + B + 3
    bar = gamma(k3) * A + (1 + gamma(k3)) * prop
    if input == "level":
        out[at, regs] = cnt > 0
        bar[at, regs] = 0
    return out, bar


def hold(name, got, ref, bar, worst):
    got = got.cpu().numpy().astype(np.float64) if torch.is_tensor(got) else got
    assert got.shape == ref.shape and np.all(np.isfinite(got)), name
    assert np.array_equal(got[bar == 0], ref[bar == 0]), name              # where the bound is 0 the value is exact
    if (bar > 0).any():
        worst[name] = max(worst.get(name, 0.0), float((np.abs(got - ref)[bar > 0] / bar[bar > 0]).max()))


_IN = {}


def stage_inputs(N, H, B):
    """(p, held, y, m) of a shape: the model and the float64 fixed points of `reference`, rounded to float32"""
    if (N, H, B) not in _IN:
        p, y0, held, ref = reference(N, H, B)
        assert np.all(ref.status == 0)
        _IN[(N, H, B)] = (p, held, ref.y.astype(np.float32), moving(p, held, B).astype(np.float32))
    return _IN[(N, H, B)]


# --------------------------------------------------------------------------- the stages at the C boundary
@pytest.mark.parametrize("N,H,B", SHAPES)
def test_each_stage_against_float64(pa, dev, N, H, B):
    """Every stage on the float32 rounding of its predecessor's float64 truth, all N regulators, both inputs, both
    reductions; the bounds are derived in inverse64, factors64 and response64."""
    from phoenix_amd import engine
    p, held, y, m = stage_inputs(N, H, B)
    P = engine_params(make_net(pa, dev, p))
    t = lambda x: torch.from_numpy(np.ascontiguousarray(x)).to(dev)      # noqa: E731
    regs = list(range(N))
    genes = torch.tensor(regs, dtype=torch.int32, device=dev)
    worst = {}
    S32 = reduced64(p, y, m).astype(np.float32)
    Z, info = engine.steady_inverse(t(S32))
    assert info.dtype == torch.int32 and not info.any()
    Z64, barZ = inverse64(S32.astype(np.float64))
    hold("Z", Z, Z64, barZ, worst)
    Z32, hid32 = Z64.astype(np.float32), parts64(p, y)[4].astype(np.float32)
    zero_info = torch.zeros(B, dtype=torch.int32, device=dev)
    for input in INPUTS:
        X, use = engine.steady_response_factors(P, t(y), t(m), t(hid32), t(Z32), zero_info, genes, input)
        Xs64, d64, barX = factors64(p, y, m, hid32.astype(np.float64), Z32.astype(np.float64), regs, input)
        assert X.shape == (B, 2 * H, N) and use.shape == (B, N) and bool((use == 1).all())
        hold("X " + input, X, Xs64, barX, worst)
        X32 = Xs64.astype(np.float32)
        ones = np.ones((B, N), np.float32)
        for mean_abs in (True, False):
            out = engine.steady_response(P, t(m), t(X32), t(ones), genes, input, mean_abs)
            ref, bar = response64(p, m, X32.astype(np.float64), ones.astype(np.float64), regs, input, mean_abs)
            hold("out %s %s" % (input, "mean_abs" if mean_abs else "mean"), out, ref, bar, worst)
    print("(%d, %d, %d): worst error / bound %s" % (N, H, B, {n: "%.3f" % v for n, v in worst.items()}))
    for name, v in worst.items():
        assert v <= 1.0, (name, v)


def test_the_inverse_reports_singular_and_non_finite_states(dev):
    from phoenix_amd import engine
    S = torch.zeros((4, 4, 4), device=dev)
    S[0] = torch.eye(4)
    S[1, 2, 1] = float("nan")
    S[2] = 0.5 * torch.eye(4)
    S[3, 0, 0], S[3, 1, 1], S[3, 2, 2], S[3, 3, 3] = 0.5, 1.0, 0.5, 0.5
    Z, info = engine.steady_inverse(S)
    assert info.tolist()[0] == 1 and info.tolist()[1] != 0 and info.tolist()[2] == 0 and info.tolist()[3] == 2
    assert torch.equal(Z[2], 2.0 * torch.eye(4, device=dev)) and not Z[:2].any() and not Z[3].any()


# --------------------------------------------------------------------------- end to end
_GPU = {}


def solved(pa, dev, N, H, B):
    """(p, held, net, steady_states at the default control) of a shape, solved once per session"""
    if (N, H, B) not in _GPU:
        p, y0, held, _ = reference(N, H, B)
        net = make_net(pa, dev, p)
        out = pa.steady_states(net, torch.from_numpy(y0).to(dev), clamp=held)
        assert out.status.tolist() == [0] * B
        _GPU[(N, H, B)] = (p, held, net, out)
    return _GPU[(N, H, B)]


def end_to_end_bound(p, y, m, regs, input, mean_abs):
    """(out64, bar): the float64 result at the float32 states y and the stages' own bounds propagated to first order --
    phx_reduced_jacobian's bound of S and the relative error of v (tests/test_steady_gpu.py) through |Z| dS |Z| into Z, that
    and the factors' own bound through |Ws|, |Wp| into X and through 1 / d into its scaling, that through |Wa| into the
    result -- and doubled for the higher orders, as 2 kappa (...) in the steady tests."""
    B, N = y.shape
    H = p["Ws"].shape[0]
    S64, _, hid64, AS, _, _, rel_v, k = kernel_truth(p, y, m, np.zeros_like(y))
    rel = np.concatenate([np.zeros((B, H)), rel_v], axis=1)
    dS = (k * (1 + rel) + rel)[:, :, None] * AS
    Z64, barZ = inverse64(S64, dS)
    Xs64, _, barX = factors64(p, y, m, hid64, Z64, regs, input, dZ=barZ, rel_v=rel_v + U)
    out64, bar = response64(p, m, Xs64, np.ones((B, len(regs))), regs, input, mean_abs, dXs=barX)
    return out64, 2 * bar


@pytest.mark.parametrize("N,H,B", SHAPES)
def test_response_against_the_reference_at_the_devices_steady_states(pa, dev, N, H, B):
    p, held, net, st = solved(pa, dev, N, H, B)
    y = st.y.cpu().numpy()
    m = moving(p, held, B).astype(np.float32)
    regs = list(range(N))
    worst, scale = {}, {}
    from phoenix_amd import engine
    P, tm = engine_params(net), torch.from_numpy(m).to(dev)
    genes = torch.tensor(regs, dtype=torch.int32, device=dev)
    for input in INPUTS:
        for reduce in ("mean_abs", "mean"):
            got = pa.steady_state_response(net, st.y, clamp=held, input=input, reduce=reduce, status=st.status)
            ref = pa.steady_state_response_reference(p, y, clamp=held, input=input, reduce=reduce)
            assert got.info.dtype == torch.int32 and got.info.tolist() == ref.info.tolist() == [0] * B
            assert got.regulators == regs and got.response.shape == (N, N) and got.response.dtype == torch.float32
            # the public function is the chain of the stages that test_each_stage_against_float64 holds one by one, to the bit
            S, _, hid = engine.reduced_jacobian(P, st.y, tm)
            Z, info = engine.steady_inverse(S)
            X, use = engine.steady_response_factors(P, st.y, tm, hid, Z, info, genes, input)
            assert torch.equal(got.response, engine.steady_response(P, tm, X, use, genes, input, reduce == "mean_abs"))
            out64, bar = end_to_end_bound(p, y, m, regs, input, reduce == "mean_abs")
            assert np.abs(out64 - ref.response).max() <= 1e-12          # the bound's own float64 chain is the reference's
            hold("%s %s" % (input, reduce), got.response, ref.response, bar, worst)
            r32 = pa.steady_state_response_reference(p, y, clamp=held, input=input, reduce=reduce, dtype=np.float32)
            scale["%s %s" % (input, reduce)] = "%.1e %.1e %.1e" % (
                np.abs(got.response.cpu().numpy() - ref.response).max(), np.abs(r32.response - ref.response).max(), bar.max())
            # the scores: the bound summed over a row, and an N-term float32 sum of the magnitudes in any order
            sc = got.scores.cpu().numpy().astype(np.float64)
            sc_bar = (bar.sum(axis=1) + gamma(N + 2) * (np.abs(ref.response) + bar).sum(axis=1)) / max(N - 1, 1)
            assert np.all(np.abs(sc - ref.scores) <= sc_bar)
    print("(%d, %d, %d): worst error / bound %s" % (N, H, B, {n: "%.1e" % v for n, v in worst.items()}))
    print("    |device - ref64|, |ref32 - ref64|, largest bound: %s" % scale)
    for name, v in worst.items():
        assert v <= 1.0, (name, v)


@pytest.mark.parametrize("N,H,B", [(130, 40, 3), (70, 97, 3)])
def test_regulator_blocks_have_the_bits_of_the_full_result(pa, dev, N, H, B):
    p, held, net, st = solved(pa, dev, N, H, B)
    rng = np.random.default_rng(N)
    for input, reduce in (("level", "mean_abs"), ("production", "mean")):
        full = pa.steady_state_response(net, st.y, clamp=held, input=input, reduce=reduce)
        again = pa.steady_state_response(net, st.y, clamp=held, input=input, reduce=reduce, regulators=range(N))
        assert torch.equal(full.response, again.response) and torch.equal(full.scores, again.scores)
        for size in (1, 63, 65 if N >= 65 else N - 1):
            regs = [int(k) for k in rng.choice(N, size, replace=False)]
            sub = pa.steady_state_response(net, st.y, clamp=held, input=input, reduce=reduce, regulators=regs)
            assert sub.regulators == regs and sub.response.shape == (size, N)
            assert torch.equal(sub.response, full.response[regs])
            # (the scores are torch's sums over the rows of the result, whose order may follow the number of rows: two
            # N-term float32 sums of the same magnitudes)
            slack = 2 * gamma(N + 2) * full.response[regs].abs().sum(dim=1) / (N - 1)
            assert bool(((sub.scores - full.scores[regs]).abs() <= slack).all())
        # blocks of 7 regulators, of 64, and one block
        for rows_bytes in (7 * B * 2 * H * 4, 64 * B * 2 * H * 4, 1):
            cut = pa.steady_state_response(net, st.y, clamp=held, input=input, reduce=reduce, rows_bytes=rows_bytes)
            assert torch.equal(cut.response, full.response)
        assert torch.equal(pa.steady_state_response(net, st.y.reshape(B, 1, N), clamp=held, input=input, reduce=reduce).response,
                           full.response)


@pytest.mark.parametrize("N,H,B", [(97, 7, 5), (70, 97, 3)])
def test_exact_values(pa, dev, N, H, B):
    p, y0, held, ref = reference(N, H, B)
    p = {k: v.copy() for k, v in p.items()}
    free = moving(p, held, B)
    always = np.nonzero(free.all(axis=0))[0]
    never = np.nonzero(~free.any(axis=0))[0]                  # genes with g <= 0
    sometimes = np.nonzero(free.any(axis=0) & ~free.all(axis=0))[0]
    assert len(never) and len(sometimes) and len(always) > 2
    zw = int(always[1])                                        # a regulator without outgoing weights
    p["Ws"][:, zw] = 0
    p["Wp"][:, zw] = 0
    net = make_net(pa, dev, p)
    y = torch.from_numpy(ref.y.astype(np.float32)).to(dev)
    diag = torch.arange(N, device=dev)
    for input in INPUTS:
        for reduce in ("mean_abs", "mean"):
            got = pa.steady_state_response(net, y, clamp=held, input=input, reduce=reduce)
            assert not got.info.any()
            R = got.response.clone()
            own = R[diag, diag].clone()
            R[diag, diag] = 0
            assert not R[:, torch.from_numpy(never).to(dev)].any()          # a target that moves in no row
            assert not R[zw].any()                                          # a regulator whose weight columns are 0
            assert R[torch.from_numpy(always).to(dev)][:, torch.from_numpy(always).to(dev)].any()
            if input == "level":
                assert bool((own == 1).all())
            else:
                assert not own[torch.from_numpy(never).to(dev)].any() and not R[torch.from_numpy(never).to(dev)].any()
                assert float(own[zw]) == 1.0                                # R[k, k] = m_k where nothing comes back
    # a target held in the only row: an exact zero off the diagonal
    b = next(b for b in range(B) if held[b])
    one = pa.steady_state_response(net, y[b:b + 1], clamp=[held[b]], input="level", reduce="mean")
    for k in held[b]:
        col = one.response[:, k].clone()
        assert float(col[k]) == 1.0
        col[k] = 0
        assert not col.any()


def test_rows_that_are_left_out(pa, dev):
    # a singular I - S, built on the host: the middle row of `singular_model`
    p, y = singular_model()
    net = make_net(pa, dev, p)
    ty = torch.from_numpy(y).to(dev)
    for input in INPUTS:
        for reduce in ("mean_abs", "mean"):
            got = pa.steady_state_response(net, ty, input=input, reduce=reduce)
            rest = pa.steady_state_response(net, ty[[0, 2]], input=input, reduce=reduce)
            assert got.info.tolist() == [0, 1, 0] and rest.info.tolist() == [0, 0]
            assert torch.equal(got.response, rest.response) and bool(got.response.abs().max() > 0)
            ref = pa.steady_state_response_reference(p, y, input=input, reduce=reduce)
            assert ref.info.tolist() == [0, 1, 0]
            out64, bar = end_to_end_bound(p, y[[0, 2]], np.ones((2, y.shape[1]), np.float32), list(range(y.shape[1])), input,
                                          reduce == "mean_abs")
            assert np.abs(out64 - ref.response).max() <= 1e-12
            hold("left out", got.response, ref.response, bar, {})
            assert np.all(np.abs(got.response.cpu().numpy() - ref.response) <= bar)
    only = pa.steady_state_response(net, ty[1:2])                  # no row is used: zeros, no division by 0
    assert only.info.tolist() == [1] and not only.response.any() and not only.scores.any()
    # a row whose status is not 0 is left out the same way, with its own code
    N, H, B = 97, 7, 5
    p, held, net, st = solved(pa, dev, N, H, B)
    status = torch.tensor([0, 1, 0, 2, 0], dtype=torch.int32, device=dev)
    got = pa.steady_state_response(net, st.y, clamp=held, status=status)
    keep = [0, 2, 4]
    rest = pa.steady_state_response(net, st.y[keep], clamp=[held[b] for b in keep])
    assert got.info.tolist() == [0, -2, 0, -2, 0] and torch.equal(got.response, rest.response)
    assert torch.equal(pa.steady_state_response(net, st.y, clamp=held, status=status.cpu().numpy()).response, got.response)


@pytest.mark.parametrize("N,H,B,b", [(37, 5, 3, 1), (96, 56, 4, 2), (70, 97, 3, 1)])
def test_cross_check_with_the_implicit_adjoint(pa, dev, N, H, B, b):
    """Row b holds a gene k.  With input="level", one state and reduce="mean", sum_j gy_j response[k, j] is dL/d(level of k)
    of L = sum_j gy_j y*_j: the quantity y0.grad[b, k] of steady_states(differentiable=True).  Both are held to the float64
    reference at the device's y*: ours under the end-to-end bound above summed with |gy| (the sum itself is taken in
    float64), the adjoint's under the bound of tests/test_steady_adjoint_gpu.py, 8 |ref32 - ref64| + gamma_B A; the two
    routes agree within the sum of the two."""
    p, y0, held = make_model(N, H, B)
    assert held[b]
    net = make_net(pa, dev, p)
    for q in net.parameters():
        q.requires_grad_(True)
    y0t = torch.from_numpy(y0[b:b + 1]).to(dev).requires_grad_(True)
    clamp = [held[b]]
    st = pa.steady_states(net, y0t, clamp=clamp, differentiable=True)
    assert st.status.tolist() == [0]
    gy = np.random.default_rng(1000 + N).standard_normal((1, N)).astype(np.float32)
    (st.y * torch.from_numpy(gy).to(dev)).sum().backward()
    ystar = st.y.detach().cpu().numpy()
    m = moving(p, clamp, 1).astype(np.float32)
    regs = [int(k) for k in held[b]]
    got = pa.steady_state_response(net, st.y.detach(), clamp=clamp, regulators=regs, input="level", reduce="mean")
    out64, bar = end_to_end_bound(p, ystar, m, regs, "level", False)
    g64 = gy[0].astype(np.float64)
    ours = got.response.cpu().numpy().astype(np.float64) @ g64
    ours_bar = bar @ np.abs(g64)
    r64 = pa.steady_states_adjoint_reference(p, ystar, gy, clamp=clamp)
    r32 = pa.steady_states_adjoint_reference(p, ystar, gy, clamp=clamp, dtype=np.float32)
    A = back64(p, ystar, None, gy, r64.q, parts64(p, ystar)[4])[1]
    theirs_bar = 8 * float(np.abs(r32.y0.astype(np.float64) - r64.y0).max()) + gamma(1) * float(A.max())
    theirs = y0t.grad.cpu().numpy().astype(np.float64)[0, regs]
    truth = r64.y0[0, regs]
    assert np.abs(out64 @ g64 - truth).max() <= 1e-12 * max(1.0, np.abs(truth).max())       # the two float64 formulas agree
    print("(%d, %d) row %d, genes %s: |ours - ref64| %s (bound %s), |adjoint - ref64| %s (bound %.1e)"
          % (N, H, b, regs, np.abs(ours - truth), ours_bar, np.abs(theirs - truth), theirs_bar))
    assert np.all(np.abs(ours - truth) <= ours_bar) and np.all(np.abs(theirs - truth) <= theirs_bar)
    assert np.all(np.abs(ours - theirs) <= ours_bar + theirs_bar)
