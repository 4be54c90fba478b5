"""In-silico knockout screens on the MI355X: `odeint_calls(clamp=...)` (phx_odeint_clamped: the CALLS + CLAMP forms of
k1_solve_fwd3 / k1_solve_fwd3c) against the model the clamp is defined by -- the same parameters with g[gene] = 0, solved
by the CPU oracle and by the engine's own `odeint` --, phx_knockout_effects against the float64 restatement of
tests/test_knockout_cpu.py, and `knockout_effects` end to end.  Run with `-m gpu`; every test prints the figures it
measured before it asserts (run with -s to see them).

The forms of the kernels each shape (N, H, B, K) of test 1 runs, as planned for 256 CUs (asserted through phx_debug_plan):
    (96, 8, 5, 6), (350, 30, 7, 5)     k1_solve_fwd3  <HALF>
    (96, 44, 5, 4)                     k1_solve_fwd3  <full last tile>
    (96, 56, 5, 4), (350, 200, 7, 3)   k1_solve_fwd3c <NBT 1, HALF, HB>
    (96, 96, 5, 4)                     k1_solve_fwd3c <NBT 1, full, HB>
    (96, 56, 5, 50)                    k1_solve_fwd3c <NBT 1, HALF, whole blocks>   (150 workgroups: no room for half blocks)
    (96, 96, 5, 50)                    k1_solve_fwd3c <NBT 1, full, whole blocks>
    (96, 56, 70, 2)                    k1_solve_fwd3c <NBT 8, HALF>                 (five trajectory tiles on four waves)
    (96, 96, 70, 2)                    k1_solve_fwd3c <NBT 8, full>
Measured on an MI355X: test 1 against the oracle <= 2.6e-6 on every call (bar 1e-5), the clamped column drifts by exactly
0; against the engine's own odeint on the zeroed module bitwise equal in every shape but the two 50-call ones (<= 1.7e-6:
a lone call of that shape plans half-block gene tiles, 50 calls do not fit them).  Scoring against float64: scores <=
7.0e-8, worst magnitude entry <= 3.4e-7, shift <= 1.5e-7 of the largest magnitude (bar 2e-5); end to end: scores <= 8.4e-8,
matrices <= 1.5e-7; genes_per_launch 1 and 8 gave identical bits.
"""
import ctypes as C

import numpy as np
import pytest
import torch

from conftest import relerr
from test_calls_grids_gpu import TOL_FIXED_CALLS, _grids
from test_gpu_parity import TOL_DOPRI, make_net, onet_of, rand_params
from test_influence_gpu import TOL, decades, max_rel
from test_knockout_cpu import reference64

pytestmark = pytest.mark.gpu

T_SOLVE = 5


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "these tests need the MI355X"
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def pa():
    import phoenix_amd
    return phoenix_amd


def _y0s(N, B, K, seed):
    rs = np.random.RandomState(seed)
    return np.stack([(rs.rand(B, 1, N).astype(np.float32) - 0.5) * (0.6 + 0.2 * (k % 4)) for k in range(K)])


def _zeroed(p, gene):
    q = dict(p)
    q["g"] = p["g"].copy()
    if gene >= 0:
        q["g"][gene] = 0.0
    return q


def _form(N, H, B, K):
    """(kernel, NBT, HALF, HB) of the launch of K calls of B rows, as prepare_fwd3 / prepare_fwd3c pick it"""
    from phoenix_amd import _lib
    lib = _lib.load()
    kern = lib.phx_debug_calls_grids_kernel_m(N, H, B * K, T_SOLVE, K, _lib.METHODS["dopri5"])
    out = (C.c_longlong * 64)()
    n = lib.phx_debug_plan(_lib.OP_ODEINT, kern, lib.phx_device_cus(), N, H, B * K, T_SOLVE, _lib.CTRL_SHARED,
                           _lib.METHODS["dopri5"], K, out)
    assert n > 21
    NB, TPW, Hc, hb, split = out[5], out[7], out[16], out[20], out[21]
    if kern == 3:
        return (3, 0, H <= 40, False)
    return (4, 1 if (TPW * NB <= 1 or split > 1) else 8, Hc <= 40, bool(hb))


# what a clamp list is made of: "m" = the gene that would move most (see the test), "neg" = a gene with g <= 0,
# "last" = N - 1 (the last, partial block), the half-block (15 / 16) and block (31 / 32) boundaries, -1 = none
SHAPES = [
    (96, 8, 5, 6, (3, 0, True, False), ["m", 0, 15, 16, -1, "neg"]),
    (350, 30, 7, 5, (3, 0, True, False), [31, 32, "m", "last", -1]),
    (96, 44, 5, 4, (3, 0, False, False), ["last", "m", "neg", -1]),
    (96, 56, 5, 4, (4, 1, True, True), ["m", 32, -1, 15]),
    (350, 200, 7, 3, (4, 1, True, True), ["m", "last", -1]),
    (96, 96, 5, 4, (4, 1, False, True), [16, "m", -1, 31]),
    (96, 56, 5, 50, (4, 1, True, False), ["m", 0, 15, 16, 31, 32, "last", "neg", -1]),
    (96, 96, 5, 50, (4, 1, False, False), ["m", 0, 15, 16, 31, 32, "last", "neg", -1]),
    (96, 56, 70, 2, (4, 8, True, False), ["m", "last"]),
    (96, 96, 70, 2, (4, 8, False, False), [16, "m"]),
]


# --------------------------------------------------------------------------- 1. clamped calls equal the g-zeroed model
@pytest.mark.parametrize("N,H,B,K,form,spec", SHAPES)
def test_clamped_calls_equal_the_model_with_a_zeroed_multiplier(pa, dev, oracle, N, H, B, K, form, spec):
    p = rand_params(N, H, seed=N + H + K, std=0.6 / np.sqrt(N))
    assert _form(N, H, B, K) == form
    y0s, tg = _y0s(N, B, K, seed=N + K), np.stack([_grids(6, T_SOLVE, np.float64)[k % 6] + 0.01 * (k // 6) for k in range(K)])
    onet = onet_of(oracle, p)
    pos, neg = np.flatnonzero(p["g"] > 0), np.flatnonzero(p["g"] <= 0)
    assert len(neg) > 0
    clamp, movers = [], []
    for k in range(K):
        s = spec[k] if k < len(spec) else (7 * k) % N
        if s == "m":       # the gene whose derivative at y0 is largest among those with a positive multiplier
            f = np.abs(oracle.rhs(onet, y0s[k])).reshape(B, N).max(axis=0)
            s = int(pos[np.argmax(f[pos])])
            movers.append(k)
        clamp.append({"neg": int(neg[len(neg) // 2]), "last": N - 1}.get(s, s))
    assert movers and -1 in clamp or K == 2
    net = make_net(pa, dev, p)
    g_before = net.gene_multipliers.detach().clone()
    y0d, td = torch.from_numpy(y0s).to(dev), torch.from_numpy(tg).to(dev)
    out = pa.odeint_calls(net, y0d, td, method="dopri5", clamp=clamp)
    assert out.shape == (K, T_SOLVE, B, 1, N)
    got = out.cpu().numpy()
    assert torch.equal(net.gene_multipliers.detach(), g_before)
    znet = make_net(pa, dev, p)
    bitwise = []
    for k in range(K):
        q = _zeroed(p, clamp[k])
        ref = oracle.odeint(onet_of(oracle, q), y0s[k], tg[k], method="dopri5")
        e_o = relerr(got[k], ref)
        with torch.no_grad():
            znet.gene_multipliers.copy_(torch.from_numpy(q["g"]).reshape(1, N))
            own = pa.odeint(znet, y0d[k], td[k], method="dopri5").cpu().numpy()
        e_e = relerr(got[k], own)
        bitwise.append(bool(np.array_equal(got[k], own)))
        hold = 0.0
        if clamp[k] >= 0:
            col = y0s[k][None, :, :, clamp[k]]
            hold = float(np.abs(got[k][..., clamp[k]] - col).max()) / max(float(np.abs(col).max()), 1e-30)
        print("call %d gene %d: oracle relerr %.3e, engine odeint relerr %.3e (bitwise %s), clamped column drift %.3e"
              % (k, clamp[k], e_o, e_e, bitwise[-1], hold))
        assert e_o < TOL_DOPRI, k
        assert e_e < TOL_DOPRI, k
        assert hold < TOL_DOPRI, k
        if k in movers:      # a condition on the inputs: an ignored clamp could not pass (the oracle supplies both sides)
            free = oracle.odeint(onet, y0s[k], tg[k], method="dopri5")
            moved = float(np.abs(free[..., clamp[k]] - ref[..., clamp[k]]).max()) / float(np.abs(ref).max())
            print("   the unclamped solve moves gene %d by %.3e of the trajectory scale" % (clamp[k], moved))
            assert moved > 100 * TOL_DOPRI
    print("clamped launch == engine odeint on the zeroed multiplier, bit for bit: %d of %d calls" % (sum(bitwise), K))


def test_clamped_calls_at_the_breast_cancer_shape(pa, dev):
    """(N, H, B) = (11165, 40, 60): gene tiles of eight blocks, 349 blocks, the last one partial -- the clamped gene in the
    first block, in the middle and in the last column, against the engine's own odeint on the zeroed module (the oracle
    takes too long here).  Also prints how much of the knockout's effect on the OTHER genes the solver tolerance is: on
    these random weights the effect is small, and a score of it carries that noise."""
    N, H, B, K, T = 11165, 40, 60, 3, 4
    p = rand_params(N, H, seed=5, std=0.6 / np.sqrt(N))
    strong = np.argsort(-p["g"])
    clamp = [int(strong[strong < 32][0]), int(strong[(strong > 5000) & (strong < 5032)][0]),
             N - 1 if p["g"][N - 1] > 0 else int(strong[strong >= N - 13][0])]
    net, znet = make_net(pa, dev, p), make_net(pa, dev, p)
    y0d = torch.from_numpy(_y0s(N, B, K, seed=4)).to(dev)
    td = torch.from_numpy(_grids(K, T, np.float64)).to(dev)
    out = pa.odeint_calls(net, y0d, td, method="dopri5", clamp=clamp)
    for k, gene in enumerate(clamp):
        with torch.no_grad():
            znet.gene_multipliers.copy_(torch.from_numpy(_zeroed(p, gene)["g"]).reshape(1, N))
            one = pa.odeint(znet, y0d[k], td[k], method="dopri5")
            free = pa.odeint(net, y0d[k], td[k], method="dopri5")
        e = relerr(out[k].cpu().numpy(), one.cpu().numpy())
        drift = float((out[k][..., gene] - y0d[k][None, ..., gene]).abs().max())
        moved = float((free[..., gene] - one[..., gene]).abs().max() / one.abs().max())
        others = torch.ones(N, dtype=torch.bool, device=dev)
        others[gene] = False
        effect = float((one - free)[1:][..., others].abs().mean())
        noise = float((out[k] - one)[1:][..., others].abs().mean())
        print("call %d gene %d: relerr %.3e, clamped column drift %.3e, unclamped moves it by %.3e; mean |effect| on the other "
              "genes %.3e, mean |launch - odeint| there %.3e" % (k, gene, e, drift, moved, effect, noise))
        assert e < TOL_DOPRI, k
        assert drift < TOL_DOPRI, k
        assert moved > 100 * TOL_DOPRI, k


# --------------------------------------------------------------------------- 2. more calls than one launch
def test_more_clamped_calls_than_one_launch_takes(pa, dev):
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
    clamp = [k % N for k in range(K)]
    out = pa.odeint_calls(net, y0d, td, method="dopri5", clamp=clamp)
    for k in (0, 1, n - 1, n, n + 1, K - 1):
        with torch.no_grad():
            znet.gene_multipliers.copy_(torch.from_numpy(_zeroed(p, clamp[k])["g"]).reshape(1, N))
            one = pa.odeint(znet, y0d[k], td[k], method="dopri5")
        e = relerr(out[k].cpu().numpy(), one.cpu().numpy())
        drift = float((out[k][..., clamp[k]] - y0d[k][None, ..., clamp[k]]).abs().max())
        print("call %d of %d (launches of %d), gene %d: relerr %.3e, clamped column drift %.3e" % (k, K, n, clamp[k], e, drift))
        assert e < TOL_DOPRI, k
        assert drift < TOL_DOPRI, k


# --------------------------------------------------------------------------- 3. neighbours
@pytest.mark.parametrize("N,H,B,K", [(350, 30, 7, 5), (96, 56, 5, 4)])
def test_a_clamped_call_leaves_its_neighbours_alone(pa, dev, N, H, B, K):
    p = rand_params(N, H, seed=N + H, std=0.6 / np.sqrt(N))
    net = make_net(pa, dev, p)
    y0d = torch.from_numpy(_y0s(N, B, K, seed=5)).to(dev)
    td = torch.from_numpy(_grids(K, T_SOLVE, np.float64)).to(dev)
    gene = int(np.argmax(p["g"]))      # the largest multiplier: holding it changes its call for sure
    plain = pa.odeint_calls(net, y0d, td, method="dopri5")
    none = pa.odeint_calls(net, y0d, td, method="dopri5", clamp=[-1] * K)
    assert torch.equal(none, plain)                    # nothing clamped: the launch without the list, bit for bit
    for j in (0, K - 1):
        clamp = [-1] * K
        clamp[j] = gene
        one = pa.odeint_calls(net, y0d, td, method="dopri5", clamp=torch.tensor(clamp, device=dev))
        for k in range(K):
            assert torch.equal(one[k], none[k]) == (k != j), (j, k)
    both = pa.odeint_calls(net, y0d, td, method="dopri5", clamp=[gene] + [-1] * (K - 2) + [gene])
    assert torch.equal(both[1:K - 1], none[1:K - 1]) and not torch.equal(both[0], none[0])


# --------------------------------------------------------------------------- 4. fallbacks
def _fallback_case(pa, dev):
    N, H, B, K, T = 96, 8, 5, 4, 4
    p = rand_params(N, H, seed=14, std=0.6 / np.sqrt(N))
    net = make_net(pa, dev, p)
    y0d = torch.from_numpy(_y0s(N, B, K, seed=9)).to(dev)
    td = torch.from_numpy(_grids(K, T, np.float64)).to(dev)
    strong = np.argsort(-p["g"])      # the genes with the largest multipliers: holding one changes its call for sure
    return N, p, net, y0d, td, [int(strong[0]), -1, int(strong[1]), int(strong[2])]


def _check_against_zeroed(pa, dev, N, p, out, y0d, td, clamp, method, tol):
    znet = make_net(pa, dev, p)
    for k, gene in enumerate(clamp):
        with torch.no_grad():
            znet.gene_multipliers.copy_(torch.from_numpy(_zeroed(p, gene)["g"]).reshape(1, N))
            one = pa.odeint(znet, y0d[k], td[k], method=method)
            free = pa.odeint(make_net(pa, dev, p), y0d[k], td[k], method=method)
        e = relerr(out[k].cpu().numpy(), one.cpu().numpy())
        print("%s call %d gene %d: relerr %.3e" % (method, k, gene, e))
        assert e < tol, k
        if gene >= 0:
            assert float((out[k][..., gene] - y0d[k][None, ..., gene]).abs().max()) < TOL_DOPRI
            assert relerr(free.cpu().numpy(), one.cpu().numpy()) > 100 * tol      # the clamp matters in this call


def test_fixed_grid_methods_solve_the_clamped_calls_one_by_one(pa, dev):
    N, p, net, y0d, td, clamp = _fallback_case(pa, dev)
    g_obj, g_val = net.gene_multipliers, net.gene_multipliers.detach().clone()
    out = pa.odeint_calls(net, y0d, td, method="rk4", clamp=clamp)
    assert net.gene_multipliers is g_obj and torch.equal(net.gene_multipliers.detach(), g_val)
    _check_against_zeroed(pa, dev, N, p, out, y0d, td, clamp, "rk4", TOL_FIXED_CALLS)
    stepped = pa.odeint_calls(net, y0d, td, method="rk4", options={"step_size": 0.05}, clamp=clamp)
    assert relerr(stepped[0].cpu().numpy(), out[0].cpu().numpy()) < 1e-2 and not torch.equal(stepped, out)
    assert float((stepped[0][..., clamp[0]] - y0d[0][None, ..., clamp[0]]).abs().max()) < TOL_DOPRI


def test_valu_engine_solves_the_clamped_calls_one_by_one(pa, dev, monkeypatch):
    from phoenix_amd import _lib
    N, p, net, y0d, td, clamp = _fallback_case(pa, dev)
    K, B, T = y0d.shape[0], y0d.shape[1], td.shape[1]
    ref = pa.odeint_calls(net, y0d, td, method="dopri5", clamp=clamp)
    g_obj, g_val = net.gene_multipliers, net.gene_multipliers.detach().clone()
    monkeypatch.setenv("PHX_ENGINE", "v0")
    pa.engine.forget_workspaces()
    assert _lib.load().phx_odeint_clamped_workspace_bytes(N, 8, B * K, T, K) == 0
    got = pa.odeint_calls(net, y0d, td, method="dopri5", clamp=clamp)
    monkeypatch.delenv("PHX_ENGINE")
    pa.engine.forget_workspaces()
    assert net.gene_multipliers is g_obj and torch.equal(net.gene_multipliers.detach(), g_val)
    e = relerr(got.cpu().numpy(), ref.cpu().numpy())
    print("PHX_ENGINE=v0 against the clamped launch: relerr %.3e" % e)
    assert e < TOL_FIXED_CALLS
    _check_against_zeroed(pa, dev, N, p, ref, y0d, td, clamp, "dopri5", TOL_DOPRI)


# --------------------------------------------------------------------------- 5. scoring
def _blocks(T, K, B, N, dev):
    base = decades((T, B, N), dev, seed=N + K)
    sol = decades((T, K * B, N), dev, seed=N + K + 1)
    g = torch.Generator(device=dev).manual_seed(N)
    sol = torch.where(torch.rand(sol.shape, device=dev, generator=g) < 0.5, sol, -sol)      # signed differences
    genes = [int(x) for x in np.random.RandomState(N).randint(0, N, K)]
    genes[0], genes[-1] = N - 1, (0 if K > 1 else N - 1)      # the first and the last column are somebody's gene
    return base, sol, genes


@pytest.mark.parametrize("T,K,B,N", [(10, 8, 60, 350), (2, 3, 7, 97), (5, 40, 5, 96), (10, 4, 1, 33)])
def test_scoring_kernel_against_float64(pa, dev, T, K, B, N):
    from phoenix_amd import engine
    base, sol, genes = _blocks(T, K, B, N, dev)
    r_sc, r_sh, r_mg = reference64(base.cpu().numpy(), sol.cpu().numpy(), genes)
    scores, shift, magnitude = engine.knockout_effects(base, sol, genes, want_matrices=True)
    assert scores.shape == (K,) and shift.shape == (K, N) and magnitude.shape == (K, N)
    e_s = max_rel(scores.cpu(), torch.from_numpy(r_sc))
    e_m = max_rel(magnitude.cpu(), torch.from_numpy(r_mg))
    e_h = float(np.abs(shift.cpu().numpy().astype(np.float64) - r_sh).max() / np.abs(r_mg).max())
    print("kernel vs float64 (T=%d K=%d B=%d N=%d): scores %.3e  magnitude (worst entry) %.3e  shift (of max magnitude) %.3e"
          % (T, K, B, N, e_s, e_m, e_h))
    assert e_s < TOL
    assert e_m < TOL
    assert e_h < TOL
    assert bool((shift.abs() <= magnitude * (1 + 1e-6)).all())      # |mean d| <= mean |d|
    # without the matrices (sums in the workspace), with one of them, and again: the same bits
    alone, n1, n2 = engine.knockout_effects(base, sol, genes)
    assert n1 is None and n2 is None and torch.equal(alone, scores)
    s2, _, m2 = engine.knockout_effects(base, sol, genes, magnitude=torch.empty_like(magnitude))
    assert torch.equal(s2, scores) and torch.equal(m2, magnitude)
    s3, h3, _ = engine.knockout_effects(base, sol, genes, shift=torch.empty_like(shift))
    assert torch.equal(s3, scores) and torch.equal(h3, shift)
    s4, h4, m4 = engine.knockout_effects(base, sol, genes, want_matrices=True)
    assert torch.equal(s4, scores) and torch.equal(h4, shift) and torch.equal(m4, magnitude)
    # the initial states (output 0) are not part of any mean, and are not read
    base[0] = float("nan")
    sol[0] = float("nan")
    s5, h5, m5 = engine.knockout_effects(base, sol, genes, want_matrices=True)
    assert torch.equal(s5, scores) and torch.equal(h5, shift) and torch.equal(m5, magnitude)
    # non-finite inputs propagate: one NaN in knockout 0's rows reaches its score and its column only
    sol[1, 0, 1 if genes[0] != 1 else 2] = float("nan")
    s6, _, m6 = engine.knockout_effects(base, sol, genes, want_matrices=True)
    assert bool(torch.isnan(s6[0])) and torch.equal(s6[1:], scores[1:]) and int(torch.isnan(m6).sum()) == 1


@pytest.mark.parametrize("T,K,B,N", [(10, 3, 60, 350), (10, 2, 7, 11165)])
def test_clamped_column_is_skipped_not_subtracted(pa, dev, T, K, B, N):
    """the case of test_influence_gpu.py::test_perturbed_column_is_skipped_not_subtracted: the clamped gene's own column
    differs by 1e6, every other by about 1e-3, so a float32 `total - column` loses the score altogether"""
    from phoenix_amd import engine
    g = torch.Generator(device=dev).manual_seed(7)
    genes = [0, N - 1, N // 2][:K]
    base = torch.rand((T, B, N), device=dev, generator=g)
    sol = (base[:, None] + 1e-3 * torch.rand((T, K, B, N), device=dev, generator=g)).reshape(T, K * B, N).contiguous()
    for k in range(K):
        sol[:, k * B:(k + 1) * B, genes[k]] = base[:, :, genes[k]] + 1e6
    r_sc, r_sh, r_mg = reference64(base.cpu().numpy(), sol.cpu().numpy(), genes)
    scores, shift, magnitude = engine.knockout_effects(base, sol, genes, want_matrices=True)
    e_s = max_rel(scores.cpu(), torch.from_numpy(r_sc))
    print("skip by index (N=%d): scores %.3e; own columns %s" % (N, e_s, [float(magnitude[k, genes[k]]) for k in range(K)]))
    assert e_s < TOL
    assert max_rel(magnitude.cpu(), torch.from_numpy(r_mg)) < TOL
    for k in range(K):        # reported as computed
        assert abs(float(magnitude[k, genes[k]]) - 1e6) < 1.0 and abs(float(shift[k, genes[k]]) - 1e6) < 1.0


# --------------------------------------------------------------------------- 6. end to end
def test_knockout_effects_end_to_end(pa, dev):
    N, H, B = 350, 30, 7
    p = rand_params(N, H, seed=N + H, std=0.6 / np.sqrt(N))
    net = make_net(pa, dev, p)
    pos = np.flatnonzero(p["g"] > 0)
    genes = [int(pos[0]), 16, 31, int(np.flatnonzero(p["g"] <= 0)[0]), N - 1]
    y0 = torch.from_numpy(np.random.RandomState(2).rand(B, 1, N).astype(np.float32) - 0.5).to(dev)
    t = torch.from_numpy(np.arange(0, 1, 0.1)).to(dev)
    g_obj, g_val = net.gene_multipliers, net.gene_multipliers.detach().clone()
    res = pa.knockout_effects(net, y0, genes=genes, value=0.0)
    assert net.gene_multipliers is g_obj and torch.equal(net.gene_multipliers.detach(), g_val)
    assert isinstance(res, pa.KnockoutEffects) and res.genes == genes
    assert res.scores.shape == (5,) and res.scores.dtype == np.float32 and res.shift.shape == (5, N) == res.magnitude.shape
    # the plain loop: one zeroed-multiplier odeint per gene against one unperturbed odeint, float64 means
    znet = make_net(pa, dev, p)
    with torch.no_grad():
        base = pa.odeint(net, y0, t, method="dopri5").double()
        for i, gene in enumerate(genes):
            znet.gene_multipliers.copy_(torch.from_numpy(_zeroed(p, gene)["g"]).reshape(1, N))
            y0k = y0.clone()
            y0k[:, 0, gene] = 0.0
            d = (pa.odeint(znet, y0k, t, method="dopri5").double() - base)[1:]
            shift, mag = d.mean(dim=(0, 1, 2)).cpu().numpy(), d.abs().mean(dim=(0, 1, 2)).cpu().numpy()
            score = float(np.delete(mag, gene).mean())
            e_s = abs(float(res.scores[i]) - score) / score
            # the matrices against the largest entry of the row (the suite's relerr): the two sides are different
            # solves, so a small mean carries the solver's noise at the scale of the large ones
            e_m, e_h = relerr(res.magnitude[i].cpu().numpy(), mag), relerr(res.shift[i].cpu().numpy(), shift) if np.abs(shift).max() else 0.0
            print("gene %d: score %.6e (loop %.6e, relative %.3e), magnitude relerr %.3e, shift relerr %.3e"
                  % (gene, res.scores[i], score, e_s, e_m, e_h))
            assert e_s < TOL and e_m < TOL and e_h < TOL, gene
    # a gene whose multiplier was off already never moved: its own column of `shift` is minus its mean starting level
    assert abs(float(res.shift[3, genes[3]]) + float(y0[:, 0, genes[3]].double().mean())) < 1e-6
    # genes_per_launch and the optional outputs change no bit
    one = pa.knockout_effects(net, y0, genes=genes, genes_per_launch=1)
    lean = pa.knockout_effects(net, y0, genes=genes, want_matrices=False)
    assert lean.shift is None and lean.magnitude is None
    assert np.array_equal(one.scores, res.scores) and np.array_equal(lean.scores, res.scores)
    assert torch.equal(one.shift, res.shift) and torch.equal(one.magnitude, res.magnitude)
    # an over-expression: per-gene levels, other scores than the knockout's
    over = pa.knockout_effects(net, y0, genes=genes[:2], value=[2.0, 3.0], want_matrices=False)
    assert np.all(np.isfinite(over.scores)) and np.all(over.scores > 0) and np.all(over.scores != res.scores[:2])
    # the scores feed the pathway tools as they are
    names, s = pa.consolidate_gene_scores(["g%d" % g for g in genes], res.scores)
    pw = pa.Pathways(["p0", "p1"], np.array([0, 2, 5], dtype=np.int64), np.array([0, 1, 0, 2, 4], dtype=np.int32), np.arange(5))
    perm = pa.pathway_permutation_test(s.astype(np.float32), pw, n_perm=64, seed=1, device=dev)
    assert perm.n_perm == 64 and bool(torch.isfinite(perm.z).all())
