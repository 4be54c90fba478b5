"""Combination knockout screens on the MI355X: `odeint_calls(clamp=<sets>)` (phx_odeint_clamped_sets: the CALLS + CLAMP
forms of k1_solve_fwd3 / k1_solve_fwd3c compare a gene against the call's set) against the model the sets are defined by --
the same parameters with g = 0 on the set, solved by the CPU oracle and by the engine's own `odeint` --,
phx_knockout_epistasis against the float64 restatement of tests/test_knockout_pairs_cpu.py, and `knockout_pairs` end to
end against the oracle.  Run with `-m gpu`; every test prints the figures it measured before it asserts (-s shows them).

The ten shapes of test 1 are those of tests/test_knockout_gpu.py, which between them run all eight CLAMP forms.
Measured on an MI355X: test 1 against the oracle <= 4.5e-6 on every call (bar 1e-5), every held column drifts by exactly
0; against the engine's own odeint on the zeroed module bitwise equal in every shape but the two 50-call ones (<= 4.1e-6).
The chunked batch: <= 9.4e-7 against odeint on the zeroed module, holding only the first gene of a row is 0.16 ... 0.70
away.  Fallbacks against the oracle: rk4 <= 1.2e-7 (bar 5e-6), PHX_ENGINE=v0 <= 2.5e-6 (bar 1e-5).  Scoring against
float64: scores <= 1.4e-7, interaction scores <= 1.2e-7, the matrices <= 2.1e-7 of the pair's largest magnitude (bar 2e-5).
End to end against the oracle, of the trajectory scale: shift / magnitude <= 4.0e-7 (bar 2e-5), interaction / interaction
magnitude <= 4.4e-7 (bar 4e-5), the oracle's largest off-pair interaction magnitude 1.0e-3 ... 1.2e-2; pairs_per_launch 1, 3
and 8 gave identical bits.
"""
import numpy as np
import pytest
import torch

from conftest import relerr
from test_calls_grids_gpu import TOL_FIXED_CALLS, _grids
from test_gpu_parity import TOL_DOPRI, make_net, onet_of, rand_params
from test_influence_gpu import TOL, decades, max_rel
from test_knockout_gpu import SHAPES, T_SOLVE, _form, _y0s
from test_knockout_pairs_cpu import reference64_pairs

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "these tests need the MI355X"
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def pa():
    import phoenix_amd
    return phoenix_amd


def _zeroed_set(p, genes):
    q = dict(p)
    q["g"] = p["g"].copy()
    for g in genes:
        if g >= 0:
            q["g"][g] = 0.0
    return q


def _set_znet(znet, p, genes):
    with torch.no_grad():
        znet.gene_multipliers.copy_(torch.from_numpy(_zeroed_set(p, genes)["g"]).reshape(1, -1))


# what a set is made of.  "mm": the two genes with a positive multiplier that would move most (see the test); "lane": two of
# one lane's eight genes of a block (gmap: 0 and 7); "quarter": different lane quarters (7, 8); "half" / "block": across the
# half-block (15 / 16) and block (31 / 32) boundaries; "tiles": different gene tiles; "last": with N - 1, in the last,
# partial block; "four": a set of four; "neg": with a gene whose g <= 0; "none": the empty set; "one": a bare int
def _set_of(case, N, neg):
    return {"lane": (0, 7), "quarter": (7, 8), "half": (15, 16), "block": (31, 32), "tiles": (3, N - 29), "last": (N - 1, 40),
            "four": (1, 17, 33, N - 1), "neg": (neg, 20), "none": (), "one": 5}[case]


ALL_CASES = ["mm", "lane", "quarter", "half", "block", "tiles", "last", "four", "neg", "none", "one"]
SPECS = {(96, 8, 5, 6): ["mm", "lane", "quarter", "four", "none", "neg"],
         (350, 30, 7, 5): ["block", "mm", "last", "four", "tiles"],
         (96, 44, 5, 4): ["last", "mm", "four", "one"],
         (96, 56, 5, 4): ["mm", "half", "none", "four"],
         (350, 200, 7, 3): ["mm", "four", "tiles"],
         (96, 96, 5, 4): ["half", "mm", "four", "block"],
         (96, 56, 5, 50): ALL_CASES,
         (96, 96, 5, 50): ALL_CASES,
         (96, 56, 70, 2): ["mm", "four"],
         (96, 96, 70, 2): ["four", "mm"]}


# --------------------------------------------------------------------------- 1. sets equal the model zeroed on the set
@pytest.mark.parametrize("N,H,B,K,form", [s[:5] for s in SHAPES])
def test_clamped_sets_equal_the_model_zeroed_on_the_set(pa, dev, oracle, N, H, B, K, form):
    p = rand_params(N, H, seed=N + H + K, std=0.6 / np.sqrt(N))
    assert _form(N, H, B, K) == form
    spec = SPECS[(N, H, B, K)]
    y0s, tg = _y0s(N, B, K, seed=N + K), np.stack([_grids(6, T_SOLVE, np.float64)[k % 6] + 0.01 * (k // 6) for k in range(K)])
    onet = onet_of(oracle, p)
    pos, neg = np.flatnonzero(p["g"] > 0), np.flatnonzero(p["g"] <= 0)
    assert len(neg) > 0
    clamp, movers = [], []
    for k in range(K):
        case = spec[k % len(spec)]
        if case == "mm":       # the two genes whose derivative at y0 is largest among those with a positive multiplier
            f = np.abs(oracle.rhs(onet, y0s[k])).reshape(B, N).max(axis=0)
            top = pos[np.argsort(-f[pos])[:2]]
            clamp.append((int(top[0]), int(top[1])))
            movers.append(k)
        else:
            clamp.append(_set_of(case, N, int(neg[len(neg) // 2])))
    sets = [(c,) if isinstance(c, int) else tuple(c) for c in clamp]
    assert movers and len(set(len(s) for s in sets)) > 1      # widths mixed within the launch
    net = make_net(pa, dev, p)
    g_before = net.gene_multipliers.detach().clone()
    y0d, td = torch.from_numpy(y0s).to(dev), torch.from_numpy(tg).to(dev)
    out = pa.odeint_calls(net, y0d, td, method="dopri5", clamp=clamp)
    assert out.shape == (K, T_SOLVE, B, 1, N)
    got = out.cpu().numpy()
    assert torch.equal(net.gene_multipliers.detach(), g_before)
    znet = make_net(pa, dev, p)
    bitwise, worst = [], [0.0, 0.0, 0.0]
    for k in range(K):
        ref = oracle.odeint(onet_of(oracle, _zeroed_set(p, sets[k])), y0s[k], tg[k], method="dopri5")
        e_o = relerr(got[k], ref)
        _set_znet(znet, p, sets[k])
        with torch.no_grad():
            own = pa.odeint(znet, y0d[k], td[k], method="dopri5").cpu().numpy()
        e_e = relerr(got[k], own)
        bitwise.append(bool(np.array_equal(got[k], own)))
        hold = 0.0
        for g in sets[k]:
            col = y0s[k][None, :, :, g]
            hold = max(hold, float(np.abs(got[k][..., g] - col).max()) / max(float(np.abs(col).max()), 1e-30))
        worst = [max(a, b) for a, b in zip(worst, (e_o, e_e, hold))]
        print("call %d set %s: oracle relerr %.3e, engine odeint relerr %.3e (bitwise %s), held columns drift %.3e"
              % (k, sets[k], e_o, e_e, bitwise[-1], hold))
        assert e_o < TOL_DOPRI, k
        assert e_e < TOL_DOPRI, k
        assert hold < TOL_DOPRI, k
        if k in movers:      # a condition on the inputs: an ignored entry could not pass (the oracle supplies both sides)
            free = oracle.odeint(onet, y0s[k], tg[k], method="dopri5")
            for g in sets[k]:
                moved = float(np.abs(free[..., g] - ref[..., g]).max()) / float(np.abs(ref).max())
                print("   the unclamped solve moves gene %d by %.3e of the trajectory scale" % (g, moved))
                assert moved > 100 * TOL_DOPRI, (k, g)
    print("worst of %d calls: oracle %.3e, engine odeint %.3e, drift %.3e; bit for bit equal to odeint on the zeroed module: %d"
          % (K, worst[0], worst[1], worst[2], sum(bitwise)))


# --------------------------------------------------------------------------- 2. bitwise equalities in one launch
@pytest.mark.parametrize("N,H,B", [(96, 8, 5), (96, 56, 5)])
def test_padding_duplicates_and_order_change_no_bit(pa, dev, N, H, B):
    from phoenix_amd import engine
    from phoenix_amd.odenet import params_of
    p = rand_params(N, H, seed=N + H, std=0.6 / np.sqrt(N))
    net = make_net(pa, dev, p)
    strong = np.argsort(-p["g"])
    a, b = int(strong[0]), int(strong[1])
    K, T = 6, T_SOLVE
    y0 = torch.from_numpy(np.random.RandomState(6).rand(B, 1, N).astype(np.float32) - 0.5).to(dev)
    t = torch.from_numpy(_grids(1, T, np.float64)[0]).to(dev)
    y0s = y0.unsqueeze(0).repeat(K, 1, 1, 1)
    # through odeint_calls: the four spellings of "hold a" in one launch, and both orders of a pair
    out = pa.odeint_calls(net, y0s, t, method="dopri5", clamp=[a, [a], [a, -1, -1, -1], [a, a], [a, b], [b, a]])
    for k in (1, 2, 3):
        assert torch.equal(out[k], out[0]), k
    assert torch.equal(out[4], out[5]) and not torch.equal(out[4], out[0])
    free = pa.odeint_calls(net, y0s[:1], t, method="dopri5")
    assert not torch.equal(out[0], free[0])
    # the lists as the kernel reads them (odeint_calls sorts a set and drops its duplicates and padding first): one launch
    # of six calls of width 4, one of width 1, and the same rows as the 2-D tensor argument
    pp = engine.params_cached(*params_of(net))
    y2, tK = y0s.reshape(K * B, N).contiguous(), t.reshape(1, T).repeat(K, 1).contiguous()

    def launch(rows):
        lst = torch.tensor(rows, dtype=torch.int32, device=dev)
        sol, status, _, _ = engine.solve_forward_clamped(pp, y2, tK, lst, 1e-7, 1e-9, 0)
        engine.raise_for_status(status)
        return sol.reshape(T, K, B, N).transpose(0, 1)

    w4 = launch([[a, -1, -1, -1], [-1, -1, a, -1], [a, a, -1, a], [a, N, -1, 1 << 20], [a, b, -1, -1], [-1, b, b, a]])
    w1 = launch([a] * K)
    w1b = launch([[a]] * K)
    w2 = launch([[a, a], [a, -1], [-1, a], [a, a], [a, b], [b, a]])
    for k in range(K):
        assert torch.equal(w1[k], w1[0]) and torch.equal(w1b[k], w1[0]), k
    for k in (0, 1, 2, 3):
        assert torch.equal(w4[k], w1[0]) and torch.equal(w2[k], w1[0]), k
    assert torch.equal(w4[4], w4[5]) and torch.equal(w2[4], w2[5]) and torch.equal(w2[4], w4[4])
    assert not torch.equal(w4[4], w1[0])
    assert torch.equal(out[0], w1[0].reshape(out[0].shape)) and torch.equal(out[4], w4[4].reshape(out[4].shape))


# --------------------------------------------------------------------------- 3. more calls than one launch
def test_the_chunk_driver_offsets_the_list_by_width_times_calls(pa, dev):
    from phoenix_amd import _lib
    N, H, B, T, K = 96, 8, 5, 4, 300
    lib = _lib.load()
    n = lib.phx_debug_calls_grids_plan(N, H, B * K, T, K, _lib.METHODS["dopri5"], None)
    assert 1 <= n < K and lib.phx_odeint_clamped_workspace_bytes(N, H, B * K, T, K) > 0
    p = rand_params(N, H, seed=13, std=0.6 / np.sqrt(N))
    net, znet = make_net(pa, dev, p), make_net(pa, dev, p)
    rs = np.random.RandomState(3)
    y0s = (rs.rand(K, B, 1, N).astype(np.float32) - 0.5) * (0.2 + rs.rand(K, 1, 1, 1).astype(np.float32) * 3)
    tg = np.stack([_grids(3, T, np.float64)[k % 3] + 0.01 * k for k in range(K)])
    y0d, td = torch.from_numpy(y0s).to(dev), torch.from_numpy(tg).to(dev)
    pos = np.flatnonzero(p["g"] > 0.3)      # two different genes per call, every call another pair, all of them matter
    every = [(int(a), int(b)) for a in pos for b in pos if a != b]
    clamp = [every[i] for i in rs.permutation(len(every))[:K]]
    assert len(set(clamp)) == K
    out = pa.odeint_calls(net, y0d, td, method="dopri5", clamp=torch.tensor(clamp, device=dev))
    for k in (0, 1, n - 1, n, n + 1, K - 1):
        _set_znet(znet, p, clamp[k])
        with torch.no_grad():
            one = pa.odeint(znet, y0d[k], td[k], method="dopri5")
            _set_znet(znet, p, clamp[k][:1])
            half = pa.odeint(znet, y0d[k], td[k], method="dopri5")
        e = relerr(out[k].cpu().numpy(), one.cpu().numpy())
        drift = max(float((out[k][..., g] - y0d[k][None, ..., g]).abs().max()) for g in clamp[k])
        other = relerr(half.cpu().numpy(), one.cpu().numpy())
        print("call %d of %d (launches of %d), set %s: relerr %.3e, held columns drift %.3e; holding only the first gene "
              "is %.3e away" % (k, K, n, clamp[k], e, drift, other))
        assert e < TOL_DOPRI, k
        assert drift < TOL_DOPRI, k
        assert other > 100 * TOL_DOPRI, k      # the second entry of the row matters: a list offset by `calls` alone fails


# --------------------------------------------------------------------------- 4. fallbacks
def _fallback_case(pa, dev):
    N, H, B, K, T = 96, 8, 5, 4, 4
    p = rand_params(N, H, seed=14, std=0.6 / np.sqrt(N))
    net = make_net(pa, dev, p)
    y0s = _y0s(N, B, K, seed=9)
    tg = _grids(K, T, np.float64)
    strong = [int(g) for g in np.argsort(-p["g"])]      # the largest multipliers: holding them changes the call for sure
    clamp = [(strong[0], strong[1]), (), (strong[2], strong[0]), (strong[1], strong[3])]
    return N, p, net, y0s, tg, clamp


def _check_against_oracle(oracle, p, out, y0s, tg, clamp, method, tol, label):
    got = out.cpu().numpy()
    for k, genes in enumerate(clamp):
        ref = oracle.odeint(onet_of(oracle, _zeroed_set(p, genes)), y0s[k], tg[k], method=method)
        e = relerr(got[k], ref)
        print("%s call %d set %s: oracle relerr %.3e" % (label, k, genes, e))
        assert e < tol, k
        for g in genes:
            assert float(np.abs(got[k][..., g] - y0s[k][None, :, :, g]).max()) < TOL_DOPRI
        if genes:      # both entries matter in this call
            part = oracle.odeint(onet_of(oracle, _zeroed_set(p, genes[:1])), y0s[k], tg[k], method=method)
            assert relerr(part, ref) > 100 * tol


def test_fixed_grid_methods_solve_the_sets_one_by_one(pa, dev, oracle):
    N, p, net, y0s, tg, clamp = _fallback_case(pa, dev)
    y0d, td = torch.from_numpy(y0s).to(dev), torch.from_numpy(tg).to(dev)
    g_obj, g_val = net.gene_multipliers, net.gene_multipliers.detach().clone()
    out = pa.odeint_calls(net, y0d, td, method="rk4", clamp=clamp)
    assert net.gene_multipliers is g_obj and torch.equal(net.gene_multipliers.detach(), g_val)
    _check_against_oracle(oracle, p, out, y0s, tg, clamp, "rk4", TOL_FIXED_CALLS, "rk4")


def test_valu_engine_solves_the_sets_one_by_one(pa, dev, oracle, monkeypatch):
    from phoenix_amd import _lib
    N, p, net, y0s, tg, clamp = _fallback_case(pa, dev)
    y0d, td = torch.from_numpy(y0s).to(dev), torch.from_numpy(tg).to(dev)
    K, B, T = y0d.shape[0], y0d.shape[1], td.shape[1]
    g_obj, g_val = net.gene_multipliers, net.gene_multipliers.detach().clone()
    monkeypatch.setenv("PHX_ENGINE", "v0")
    pa.engine.forget_workspaces()
    assert _lib.load().phx_odeint_clamped_workspace_bytes(N, 8, B * K, T, K) == 0
    got = pa.odeint_calls(net, y0d, td, method="dopri5", clamp=clamp)
    monkeypatch.delenv("PHX_ENGINE")
    pa.engine.forget_workspaces()
    assert net.gene_multipliers is g_obj and torch.equal(net.gene_multipliers.detach(), g_val)
    _check_against_oracle(oracle, p, got, y0s, tg, clamp, "dopri5", TOL_DOPRI, "PHX_ENGINE=v0")


# --------------------------------------------------------------------------- 5. scoring
def _pair_lists(K, G, seed):
    """K different unordered pairs of G singles, in both orientations"""
    every = [(i, j) for i in range(G) for j in range(i + 1, G)]
    rs = np.random.RandomState(seed)
    pick = [every[i] for i in rs.permutation(len(every))[:K]]
    assert len(pick) == K
    pick = [(j, i) if k % 2 else (i, j) for k, (i, j) in enumerate(pick)]
    return [p[0] for p in pick], [p[1] for p in pick]


def _pair_blocks(T, K, G, B, N, dev):
    """base, singles and a pair block = base + d_a + d_b + a planted non-additive term of the size of d_a"""
    base = decades((T, B, N), dev, seed=N + K)
    gen = torch.Generator(device=dev).manual_seed(N + G)

    def signed(x):
        return torch.where(torch.rand(x.shape, device=dev, generator=gen) < 0.5, x, -x)

    d1 = signed(decades((T, G, B, N), dev, seed=N + K + 1))
    singles = (base[:, None] + d1).reshape(T, G * B, N).contiguous()
    ia, ib = _pair_lists(K, G, seed=N)
    d1 = singles.reshape(T, G, B, N) - base[:, None]      # as float32 holds them
    planted = signed(decades((T, K, B, N), dev, seed=N + K + 2)) * d1[:, ia].abs().mean()
    sol = (base[:, None] + d1[:, ia] + d1[:, ib] + planted).reshape(T, K * B, N).contiguous()
    # the first and the last column are somebody's gene
    genes = [N - 1] + [1 + int(x) for x in np.random.RandomState(N).permutation(N - 2)[:G - 2]] + [0]
    assert len(set(genes)) == G
    return base, singles, sol, ia, ib, genes


NAMES = ("scores", "interaction_scores", "shift", "magnitude", "interaction", "interaction_magnitude")


@pytest.mark.parametrize("T,K,G,B,N", [(10, 6, 4, 60, 350), (2, 3, 3, 7, 97), (5, 40, 10, 5, 96), (10, 1, 2, 1, 33)])
def test_epistasis_kernel_against_float64(pa, dev, T, K, G, B, N):
    from phoenix_amd import engine
    base, singles, sol, ia, ib, genes = _pair_blocks(T, K, G, B, N, dev)
    ref = reference64_pairs(base.cpu().numpy(), singles.cpu().numpy(), sol.cpu().numpy(), ia, ib, genes)
    got = engine.knockout_epistasis(base, singles, sol, ia, ib, genes, want_matrices=True)
    assert all(x.shape == (K,) for x in got[:2]) and all(x.shape == (K, N) for x in got[2:])
    assert float(ref[5].min()) > 0 and float(ref[1].min()) > 1e-3 * float(ref[0].min())      # the planted term is there
    e_sc = [max_rel(got[i].cpu(), torch.from_numpy(ref[i])) for i in (0, 1)]
    top = np.abs(ref[3]).max(axis=1, keepdims=True)      # each pair's largest magnitude entry
    e_mx = [float((np.abs(got[i].cpu().numpy().astype(np.float64) - ref[i]) / top).max()) for i in (2, 3, 4, 5)]
    print("kernel vs float64 (T=%d K=%d G=%d B=%d N=%d): scores %.3e, interaction scores %.3e; of the pair's largest magnitude: "
          "shift %.3e magnitude %.3e interaction %.3e interaction magnitude %.3e" % ((T, K, G, B, N) + tuple(e_sc) + tuple(e_mx)))
    for e in e_sc + e_mx:
        assert e < TOL
    assert bool((got[2].abs() <= got[3] * (1 + 1e-6)).all()) and bool((got[4].abs() <= got[5] * (1 + 1e-6)).all())
    # a second call, and calls without the matrices (sums in the workspace) or with some of them: the same bits
    again = engine.knockout_epistasis(base, singles, sol, ia, ib, genes, want_matrices=True)
    assert all(torch.equal(x, y) for x, y in zip(again, got))
    lean = engine.knockout_epistasis(base, singles, sol, ia, ib, genes)
    assert all(x is None for x in lean[2:]) and torch.equal(lean[0], got[0]) and torch.equal(lean[1], got[1])
    for keep in ((2, 5), (3,), (4,)):
        out = [None] * 6
        for i in keep:
            out[i] = torch.empty_like(got[i])
        some = engine.knockout_epistasis(base, singles, sol, ia, ib, genes, out=out)
        assert torch.equal(some[0], got[0]) and torch.equal(some[1], got[1])
        for i in range(2, 6):
            assert (some[i] is None) if i not in keep else torch.equal(some[i], got[i]), (keep, i)
    # the K pairs split over two calls, each with its own rows of sol
    if K > 1:
        k1 = K // 2 + 1 if K > 2 else 1
        rows = sol.reshape(T, K, B, N)
        for lo, hi in ((0, k1), (k1, K)):
            part = engine.knockout_epistasis(base, singles, rows[:, lo:hi].reshape(T, (hi - lo) * B, N).contiguous(),
                                             ia[lo:hi], ib[lo:hi], genes, want_matrices=True)
            for i in range(6):
                assert torch.equal(part[i], got[i][lo:hi]), (NAMES[i], lo, hi)
    # (a, b) and (b, a): no bit changes
    swapped = engine.knockout_epistasis(base, singles, sol, ib, ia, genes, want_matrices=True)
    assert all(torch.equal(x, y) for x, y in zip(swapped, got))
    # the initial states (output 0) are not part of any mean, and are not read
    for x in (base, singles, sol):
        x[0] = float("nan")
    nan0 = engine.knockout_epistasis(base, singles, sol, ia, ib, genes, want_matrices=True)
    assert all(torch.equal(x, y) for x, y in zip(nan0, got))
    # non-finite inputs propagate: one NaN in pair 0's rows reaches its scores and its column only
    held = (genes[ia[0]], genes[ib[0]])
    col = next(c for c in range(N) if c not in held)
    sol[1, 0, col] = float("nan")
    bad = engine.knockout_epistasis(base, singles, sol, ia, ib, genes, want_matrices=True)
    assert bool(torch.isnan(bad[0][0])) and bool(torch.isnan(bad[1][0]))
    assert torch.equal(bad[0][1:], got[0][1:]) and torch.equal(bad[1][1:], got[1][1:])
    assert all(int(torch.isnan(bad[i]).sum()) == 1 and bool(torch.isnan(bad[i][0, col])) for i in range(2, 6))


@pytest.mark.parametrize("T,K,B,N", [(10, 3, 60, 350), (10, 2, 7, 11165)])
def test_held_columns_are_skipped_not_subtracted(pa, dev, T, K, B, N):
    """the case of test_knockout_gpu.py::test_clamped_column_is_skipped_not_subtracted with both own columns dominating:
    they differ by 1e6 in the pair and in their own single, every other column by about 1e-3, so a float32
    `total - column - column` loses both scores altogether.  Every pair has two singles of its own, so that what is
    planted in one pair's held columns is in no other pair's sums."""
    from phoenix_amd import engine
    g = torch.Generator(device=dev).manual_seed(7)
    genes = [0, N - 1, N // 2, 17, 33, 5][:2 * K]
    G = len(genes)
    ia, ib = [2 * k for k in range(K)], [2 * k + 1 for k in range(K)]
    base = torch.rand((T, B, N), device=dev, generator=g)
    singles = (base[:, None] + 1e-3 * torch.rand((T, G, B, N), device=dev, generator=g)).reshape(T, G * B, N).contiguous()
    sol = (base[:, None] + 1e-3 * torch.rand((T, K, B, N), device=dev, generator=g)).reshape(T, K * B, N).contiguous()
    for i in range(G):
        singles[:, i * B:(i + 1) * B, genes[i]] = base[:, :, genes[i]] + 1e6
    for k in range(K):
        for i in (ia[k], ib[k]):
            sol[:, k * B:(k + 1) * B, genes[i]] = base[:, :, genes[i]] + 1e6
        # on column a, d_ab = d_a = 1e6 and e = -d_b[a]: let it dominate the interaction sums too
        singles[:, ib[k] * B:(ib[k] + 1) * B, genes[ia[k]]] = base[:, :, genes[ia[k]]] - 1e6
    ref = reference64_pairs(base.cpu().numpy(), singles.cpu().numpy(), sol.cpu().numpy(), ia, ib, genes)
    got = engine.knockout_epistasis(base, singles, sol, ia, ib, genes, want_matrices=True)
    e_s, e_i = max_rel(got[0].cpu(), torch.from_numpy(ref[0])), max_rel(got[1].cpu(), torch.from_numpy(ref[1]))
    print("skip by index (N=%d): scores %.3e, interaction scores %.3e; own columns of magnitude %s, of interaction magnitude %s"
          % (N, e_s, e_i, [float(got[3][k, genes[ia[k]]]) for k in range(K)], [float(got[5][k, genes[ia[k]]]) for k in range(K)]))
    assert e_s < TOL
    assert e_i < TOL
    top = np.abs(ref[3]).max(axis=1, keepdims=True)      # the matrices: of each pair's largest magnitude entry
    for i in (2, 3, 4, 5):
        assert float((np.abs(got[i].cpu().numpy().astype(np.float64) - ref[i]) / top).max()) < TOL, NAMES[i]
    for k in range(K):        # reported as computed
        for i in (ia[k], ib[k]):
            assert abs(float(got[3][k, genes[i]]) - 1e6) < 1.0 and abs(float(got[2][k, genes[i]]) - 1e6) < 1.0
        assert abs(float(got[5][k, genes[ia[k]]]) - 1e6) < 1.0 and abs(float(got[4][k, genes[ia[k]]]) - 1e6) < 1.0


# --------------------------------------------------------------------------- 6. end to end
@pytest.mark.parametrize("N,H,B,std", [(96, 8, 5, 2.0), (350, 30, 7, 2.0), (96, 56, 5, 0.6)])
def test_knockout_pairs_end_to_end_against_the_oracle(pa, dev, oracle, N, H, B, std):
    p = rand_params(N, H, seed=N + H, std=std / np.sqrt(N))
    net, onet = make_net(pa, dev, p), onet_of(oracle, p)
    y0 = np.random.RandomState(1).rand(B, 1, N).astype(np.float32) - 0.5
    t = np.arange(0, 1, 0.1)
    pos = np.flatnonzero(p["g"] > 0)
    f = np.abs(oracle.rhs(onet, y0)).reshape(B, N).max(axis=0)
    genes = [int(g) for g in pos[np.argsort(-f[pos])[:3]]]      # positive multiplier, largest |f(y0)|
    value = 2.0
    y0d = torch.from_numpy(y0).to(dev)
    g_obj, g_val = net.gene_multipliers, net.gene_multipliers.detach().clone()
    res = pa.knockout_pairs(net, y0d, genes=genes, value=value)
    assert net.gene_multipliers is g_obj and torch.equal(net.gene_multipliers.detach(), g_val)
    assert isinstance(res, pa.KnockoutPairs) and res.genes == genes and isinstance(res.singles, pa.KnockoutEffects)
    pairs = [(genes[0], genes[1]), (genes[0], genes[2]), (genes[1], genes[2])]
    assert res.pairs == pairs and res.singles.genes == genes
    assert res.scores.shape == (3,) == res.interaction_scores.shape and res.scores.dtype == np.float32 == res.interaction_scores.dtype
    assert all(x.shape == (3, N) for x in (res.shift, res.magnitude, res.interaction, res.interaction_magnitude))

    # the oracle's side: four solves per pair on the zeroed models, float64 means
    def solve(held):
        y = y0.copy()
        for g in held:
            y[:, 0, g] = value
        return oracle.odeint(onet_of(oracle, _zeroed_set(p, held)), y, t, method="dopri5").reshape(len(t), B, N)

    base = solve(())
    one = [solve((g,)) for g in genes]
    two = [solve(pr) for pr in pairs]
    ref = reference64_pairs(base, np.concatenate(one, axis=1), np.concatenate(two, axis=1), [0, 0, 1], [1, 2, 2], genes)
    s = float(np.abs(base).max())      # the trajectory scale: each of the four solves is within TOL_DOPRI of it
    for k, pr in enumerate(pairs):
        keep = np.ones(N, bool)
        keep[list(pr)] = False
        signal = float(ref[5][k, keep].max()) / s
        print("pair %s: the oracle's largest off-pair interaction magnitude is %.3e of the trajectory scale" % (pr, signal))
        assert signal > 100 * TOL_DOPRI, pr      # a condition on the inputs: the interaction is above the solver's noise

    def errors(r, label):
        e = [float(np.abs(x.cpu().numpy().astype(np.float64) - y).max()) / s
             for x, y in zip((r.shift, r.magnitude, r.interaction, r.interaction_magnitude), ref[2:])]
        e_sc = [float(np.abs(x.astype(np.float64) - y).max()) / s for x, y in zip((r.scores, r.interaction_scores), ref[:2])]
        one_sc = np.array([np.delete(np.abs(o - base)[1:].mean(axis=(0, 1)), g).mean() for o, g in zip(one, genes)])
        e_1 = float(np.abs(r.singles.scores.astype(np.float64) - one_sc).max()) / s
        print("%s (N=%d H=%d) of the trajectory scale: shift %.3e magnitude %.3e interaction %.3e interaction magnitude %.3e; "
              "scores %.3e interaction scores %.3e; singles' scores %.3e" % ((label, N, H) + tuple(e) + tuple(e_sc) + (e_1,)))
        assert e[0] < 2 * TOL_DOPRI and e[1] < 2 * TOL_DOPRI
        assert e[2] < 4 * TOL_DOPRI and e[3] < 4 * TOL_DOPRI
        assert e_sc[0] < 2 * TOL_DOPRI and e_sc[1] < 4 * TOL_DOPRI      # means of those entries
        assert e_1 < 2 * TOL_DOPRI      # a single's score: a mean of differences of two solves

    errors(res, "pairs_per_launch 8")
    # pairs_per_launch 1 and 3
    r1 = pa.knockout_pairs(net, y0d, genes=genes, value=value, pairs_per_launch=1)
    r3 = pa.knockout_pairs(net, y0d, genes=genes, value=value, pairs_per_launch=3)
    errors(r1, "pairs_per_launch 1")
    errors(r3, "pairs_per_launch 3")
    same = all(np.array_equal(a, b) for a, b in ((r1.scores, r3.scores), (r1.interaction_scores, r3.interaction_scores))) and \
        all(torch.equal(a, b) for a, b in ((r1.shift, r3.shift), (r1.magnitude, r3.magnitude), (r1.interaction, r3.interaction),
                                          (r1.interaction_magnitude, r3.interaction_magnitude)))
    print("pairs_per_launch 1 and 3 bitwise equal: %s" % same)
    assert np.array_equal(r3.scores, res.scores) and torch.equal(r3.interaction, res.interaction)      # 3 pairs: one block both times
    # explicit pairs, the other order, no matrices
    lean = pa.knockout_pairs(net, y0d, pairs=[(genes[2], genes[1])], value=value, want_matrices=False)
    assert lean.genes == sorted(genes[1:]) and lean.pairs == [(genes[2], genes[1])]
    assert lean.shift is None and lean.interaction is None and lean.singles.shift is None
    assert abs(float(lean.interaction_scores[0]) - float(ref[1][2])) / s < 4 * TOL_DOPRI
