"""CPU-only checks of the Hill simulator's steady states (phx_hill_steady, include/phoenix_hip.h; `HillSystem.block_structure`
/ `steady_states` / `knockout_steady_states`, `steady_state_recovery`): the symbol exists, the schedule
is the condensation of the regulatory graph, the block substitution is a solve of (sigma I - J) delta = f, the numpy iteration
that tests/test_hillss_gpu.py holds the kernel to converges in the measured number of steps, every refusal answers before a
device call, and the recovery scores on planted arrays."""
import collections

import numpy as np
import pytest
import torch

from conftest import load_golden
from test_abi_cpu import _declared_symbols
from test_hillko_cpu import cpu_system, gene_with_descendants
from test_simulator_cpu import _system, synthetic_states

BAD_ARG = 4
SYNTHETIC = (12, 24, 40, 64, 96)
LARGEST = {12: 9, 24: 17, 40: 17, 64: 38, 96: 57}       # the feedback component of synthetic_network(N)
_CASES = {}


def shipped(fixture):
    return _system(load_golden(fixture), "cpu")


def case(name):
    """(system on the CPU, x0 float32 [B, N], clamp or None, frozen or None) of a test case, cached.  "g11": the shipped
    350-gene system, 8 rows of sample_initial(seed 0); "syn<N>": synthetic_network(N), 6 rows of synthetic_states, with a
    gene held in row 1, two in row 2 and (N = 40) a frozen gene"""
    if name not in _CASES:
        if name == "g11":
            sys_ = shipped("g11_hill")
            _CASES[name] = (sys_, sys_.sample_initial(8, rng=np.random.default_rng(0)), None, None)
        else:
            N = int(name[3:])
            sys_, info = cpu_system(N)
            g = gene_with_descendants(sys_, info)
            other = next(j for j in range(N) if j != g and not info["is_input"][j])
            clamp = [(), (g,), (other, g), (), -1, ()]
            frozen = None
            if N == 40:
                frozen = np.zeros(N, bool)
                frozen[next(j for j in range(N) if j not in (g, other) and not info["is_input"][j])] = True
            _CASES[name] = (sys_, synthetic_states(N, 6, info), clamp, frozen)
    return _CASES[name]


_REFERENCE = {}


def reference(name):
    """the float64 fixed points of a case: `steady_states_reference` at tol 1e-12 with the dense solve, solved once"""
    from phoenix_amd.simulator import steady_states_reference
    if name not in _REFERENCE:
        sys_, x0, clamp, frozen = case(name)
        _REFERENCE[name] = steady_states_reference(sys_, x0, clamp=clamp, frozen=frozen, tol=1e-12, max_iter=40)
    return _REFERENCE[name]


def moving(name):
    """bool [B, N]: the genes that move in each row of a case"""
    sys_, x0, clamp, frozen = case(name)
    free = np.repeat(~sys_.is_input[None, :], len(x0), axis=0)
    for b, held in enumerate(clamp or ()):
        for g in ([held] if isinstance(held, int) else held):
            if g >= 0:
                free[b, g] = False
    if frozen is not None:
        free &= ~frozen[None, :]
    return free


def dense_jacobian(sys_, x):
    """float64 [B, N, N] of `jacobian_reference`: entry (b, target, regulator)"""
    from phoenix_amd.simulator import jacobian_reference
    pat = sys_.jacobian_pattern()
    J = np.zeros((len(x), sys_.N, sys_.N))
    J[:, pat.target, pat.regulator] = jacobian_reference(sys_, x)
    return J


# --------------------------------------------------------------------------- the C ABI
def test_new_symbols_are_exported_and_declared():
    from phoenix_amd import _lib
    lib = _lib.load()
    for name in ("phx_hill_steady", "phx_hill_steady_lds_bytes"):
        assert name in _lib.EXPORTS and name in _declared_symbols() and hasattr(lib, name), name
    assert lib.phx_abi_version() == 7       # an additive change


def _call(lib, largest=3, E=40, n_comp=10, n_level=3, R=2, N=12, tol=1e-5, max_iter=5, tau0=1.0, **ptr):
    """phx_hill_steady with made-up device addresses: only calls that must return before touching the device"""
    names = ("code", "off", "len_", "consts", "eptr", "ereg", "order", "comp_ptr", "level_ptr", "x0", "moving", "x", "residual",
             "iterations", "status", "tau")
    a = {n: ptr.get(n, 0x1000 * (i + 1)) for i, n in enumerate(names)}
    return lib.phx_hill_steady(a["code"], a["off"], a["len_"], a["consts"], a["eptr"], a["ereg"], E, a["order"], a["comp_ptr"],
                               n_comp, a["level_ptr"], n_level, largest, a["x0"], a["moving"], R, N, tol, max_iter, tau0, a["x"],
                               a["residual"], a["iterations"], a["status"], a["tau"], None)


def test_refusals_with_nothing_launched():
    from phoenix_amd import _lib
    lib = _lib.load()
    for name in ("code", "off", "len_", "consts", "eptr", "ereg", "order", "comp_ptr", "level_ptr", "x0", "x", "residual",
                 "iterations", "status", "tau"):
        assert _call(lib, **{name: None}) == BAD_ARG, name
    assert _call(lib, R=0) == BAD_ARG and _call(lib, R=-1) == BAD_ARG and _call(lib, max_iter=-1) == BAD_ARG
    assert _call(lib, N=0) == BAD_ARG and _call(lib, E=-1) == BAD_ARG
    for tol in (float("nan"), float("inf"), -1e-9):
        assert _call(lib, tol=tol) == BAD_ARG, tol
    for tau0 in (0.0, -1.0, float("nan")):
        assert _call(lib, tau0=tau0) == BAD_ARG, tau0
    assert _call(lib, N=100, n_comp=36, largest=65) == BAD_ARG            # a component above PHX_HILL_SCC_MAX
    assert _call(lib, N=3000, E=9000, n_comp=3000) == BAD_ARG             # vectors beyond the LDS budget
    assert _call(lib, n_comp=13) == BAD_ARG and _call(lib, n_level=11) == BAD_ARG and _call(lib, largest=0) == BAD_ARG
    lds = lib.phx_hill_steady_lds_bytes
    assert lds(690, 1672, 64) == 8 * (64 * 64 + 64) + 4 * (5 * 690 + 1672 + 6) <= 80 * 1024     # two workgroups on a CU's 160 KiB
    assert lds(690, 1672, 3) == 8 * 12 + 4 * (5 * 690 + 1672 + 6) and lds(350, 900, 1) == 4 * (5 * 350 + 900 + 6)
    assert lds(100, 300, 65) == 0 and lds(3000, 9000, 3) == 0 and lds(0, 0, 1) == 0 and lds(5, 9, 6) == 0


# --------------------------------------------------------------------------- the schedule
def check_schedule(sys_):
    from scipy.sparse import csr_matrix
    from scipy.sparse.csgraph import connected_components
    blk, pat, N = sys_.block_structure(), sys_.jacobian_pattern(), sys_.N
    assert blk is sys_.block_structure()                                    # cached
    assert blk.order.dtype == blk.comp_ptr.dtype == blk.level_ptr.dtype == np.int32
    assert sorted(blk.order.tolist()) == list(range(N))
    C_, L = len(blk.comp_ptr) - 1, len(blk.level_ptr) - 1
    assert blk.comp_ptr[0] == 0 and blk.comp_ptr[-1] == N and np.all(np.diff(blk.comp_ptr) >= 1)
    assert blk.level_ptr[0] == 0 and blk.level_ptr[-1] == C_ and np.all(np.diff(blk.level_ptr) >= 1)
    assert blk.largest == int(np.diff(blk.comp_ptr).max())
    off = pat.regulator != pat.target
    graph = csr_matrix((np.ones(off.sum()), (pat.regulator[off], pat.target[off])), shape=(N, N))
    n, label = connected_components(graph, directed=True, connection="strong")
    assert n == C_
    comp_of, level_of = np.empty(N, np.int64), np.empty(N, np.int64)
    for l in range(L):
        for c in range(blk.level_ptr[l], blk.level_ptr[l + 1]):
            members = blk.order[blk.comp_ptr[c]:blk.comp_ptr[c + 1]]
            assert len(set(label[members].tolist())) == 1                   # one component of scipy's
            comp_of[members], level_of[members] = c, l
    assert len(set(zip(comp_of.tolist(), label.tolist()))) == C_            # ... and the other way round
    want = np.zeros(C_, np.int64)
    for r, t in zip(pat.regulator[off].tolist(), pat.target[off].tolist()):
        assert comp_of[r] == comp_of[t] or level_of[r] < level_of[t], (r, t)
        if comp_of[r] != comp_of[t]:
            want[comp_of[t]] = max(want[comp_of[t]], level_of[r] + 1)
    assert np.array_equal(want[comp_of], level_of)                          # 1 + the highest level of a regulating component
    for g in np.flatnonzero(sys_.is_input):
        c = comp_of[g]
        assert level_of[g] == 0 and blk.comp_ptr[c + 1] - blk.comp_ptr[c] == 1
    return C_, blk.largest


def test_block_structure_of_the_shipped_systems():
    assert check_schedule(shipped("g11_hill")) == (348, 3)
    assert check_schedule(shipped("g13_hill690")) == (688, 3)


@pytest.mark.parametrize("N", SYNTHETIC + (350,))
def test_block_structure_of_the_synthetic_networks(N):
    _, largest = check_schedule(cpu_system(N)[0])
    if N in LARGEST:
        assert largest == LARGEST[N]
    else:
        assert largest > 64


# --------------------------------------------------------------------------- the substitution
@pytest.mark.parametrize("name", ["g11", "syn12", "syn40", "syn96"])
def test_block_substitution_is_a_solve(name):
    from phoenix_amd.simulator import block_substitution, jacobian_reference, rates_reference
    sys_, x0, _, _ = case(name)
    x = x0[:2].astype(np.float64)
    free = ~sys_.is_input
    f = np.where(free, rates_reference(sys_, x), 0.0)
    Jv, Jd = jacobian_reference(sys_, x), dense_jacobian(sys_, x)
    worst = 0.0
    for sigma in (2.0, 0.1, 0.0):
        for b in range(len(x)):
            A = -Jd[b]
            A[np.arange(sys_.N), np.arange(sys_.N)] += np.where(free, sigma, 1.0)
            want = np.linalg.solve(A, f[b])
            got, bad = block_substitution(sys_, Jv[b], f[b], sigma, free)
            assert not bad and got.dtype == np.float64 and np.all(got[~free] == 0)
            worst = max(worst, float(np.abs(got - want).max() / np.abs(want).max()))
    print("%s: block substitution against np.linalg.solve, worst relative error %.2e" % (name, worst))
    assert worst <= 1e-12


def test_block_substitution_reports_a_zero_divisor_and_a_singular_block():
    from phoenix_amd.simulator import HillSystem, block_substitution, _lu_solve
    sys_ = HillSystem(["B", "A"], ["input gene", "((0.9 * fAct(B, 0.3, 2)) * 1 - 0 * A) / 1"], device="cpu")
    pat = sys_.jacobian_pattern()
    J = np.where(pat.regulator == pat.target, 0.0, 0.5)
    free = ~sys_.is_input
    assert block_substitution(sys_, J, np.array([0.0, 0.3]), 0.0, free)[1]          # sigma - J_AA = 0
    d, bad = block_substitution(sys_, J, np.array([0.0, 0.3]), 0.5, free)
    assert not bad and d.tolist() == [0.0, 0.6]
    assert _lu_solve(np.array([[1.0, 2.0], [2.0, 4.0]]), np.ones(2))[1]
    assert _lu_solve(np.array([[1.0, np.nan], [2.0, 4.0]]), np.ones(2))[1]
    x, bad = _lu_solve(np.array([[0.0, 2.0], [4.0, 1.0]]), np.array([2.0, 5.0]))    # needs the row exchange
    assert not bad and np.allclose(x, [1.0, 1.0], rtol=0, atol=1e-15)


# --------------------------------------------------------------------------- the iteration
@pytest.mark.parametrize("name,steps", [("g11", 8)] + [("syn%d" % n, 15) for n in SYNTHETIC])
def test_reference_converges_in_the_measured_number_of_steps(name, steps):
    from phoenix_amd.simulator import rates_reference, steady_states_reference
    sys_, x0, clamp, frozen = case(name)
    free = moving(name)
    res = {s: steady_states_reference(sys_, x0, clamp=clamp, frozen=frozen, tol=1e-9, solve=s) for s in ("dense", "blocks")}
    for s, r in res.items():
        print("%s, solve=%s: steps %s, residual up to %.1e" % (name, s, r.iterations.tolist(), r.residual.max()))
        assert r.status.tolist() == [0] * len(x0) and r.iterations.max() <= steps and r.residual.max() <= 1e-9
        assert r.y.dtype == np.float64 and r.reduced is None
        assert np.array_equal(r.y[~free], x0.astype(np.float64)[~free])            # held, frozen and input genes: x0's bits
        assert np.array_equal(np.where(free, np.abs(rates_reference(sys_, r.y)), 0).max(axis=1), r.residual)
    assert np.abs(res["dense"].y - res["blocks"].y).max() <= 1e-10
    tight = reference(name)
    assert tight.status.tolist() == [0] * len(x0) and np.abs(tight.y - res["dense"].y).max() <= 1e-6


def test_reference_control():
    from phoenix_amd.simulator import HillSystem, steady_states_reference
    sys_, x0, clamp, frozen = case("syn24")
    none = steady_states_reference(sys_, x0, clamp=clamp, tol=1e-9, max_iter=0)
    assert np.array_equal(none.y, x0.astype(np.float64)) and none.status.tolist() == [1] * 6 and not none.iterations.any()
    done = steady_states_reference(sys_, reference("syn24").y, clamp=clamp, tol=1e-9, max_iter=0)
    assert done.status.tolist() == [0] * 6
    two = steady_states_reference(sys_, x0, clamp=clamp, tol=1e-9, max_iter=2)
    assert two.status.tolist() == [1] * 6 and two.iterations.tolist() == [2] * 6
    f32 = steady_states_reference(sys_, x0, clamp=clamp, tol=1e-5, dtype=np.float32, solve="blocks")
    assert f32.y.dtype == np.float32 and f32.status.tolist() == [0] * 6 and np.abs(f32.y - reference("syn24").y).max() < 1e-3
    # Newton on a regulated gene without decay: sigma - J_AA = 0, status 2 at the first step, the state untouched
    flat = HillSystem(["B", "A"], ["input gene", "((0.9 * fAct(B, 0.3, 2)) * 1 - 0 * A) / 1"], device="cpu")
    x = np.array([[0.6, 0.2]])
    for solve in ("dense", "blocks"):
        r = steady_states_reference(flat, x, tau0=float("inf"), solve=solve)
        assert r.status.tolist() == [2] and r.iterations.tolist() == [1] and np.array_equal(r.y, x)


# --------------------------------------------------------------------------- host-side argument checks
def test_steady_states_check_their_arguments_on_the_host():
    sys_, _ = cpu_system(12)
    x0 = torch.zeros(2, 12)
    for kw in (dict(tol=-1.0), dict(tol=float("inf")), dict(max_iter=-1), dict(max_iter=2.5), dict(tau0=0.0), dict(method="lu"),
               dict(clamp=[0]), dict(clamp=[(0, 1, 2, 3, 4), ()]), dict(clamp=[12, 0]), dict(frozen=torch.zeros(3, 12, dtype=torch.bool)),
               dict(frozen=torch.zeros(12))):
        with pytest.raises((ValueError, TypeError), match="steady_states"):
            sys_.steady_states(x0, **kw)
    with pytest.raises(ValueError, match="steady_states"):
        sys_.steady_states(torch.zeros(2, 11))
    with pytest.raises(ValueError, match="steady_states"):
        sys_.steady_states(torch.zeros(2, 12, dtype=torch.float64))
    big, _ = cpu_system(350)
    with pytest.raises(ValueError, match="largest component"):
        big.steady_states(torch.zeros(2, 350), method="blocks")
    assert big._steady_control("steady_states", 1e-5, 50, 1.0, None) == "dense"
    assert sys_._steady_control("steady_states", 1e-5, 50, 1.0, None) == "blocks"
    for method in (None, "blocks", "dense"):
        with pytest.raises(RuntimeError, match="no CPU path|must live on the GPU"):
            sys_.steady_states(x0, method=method)
    for kw, exc in ((dict(genes=[12]), ValueError), (dict(genes=[]), ValueError), (dict(genes=[0.5]), TypeError),
                    (dict(genes=[0, 1], value=[0.0]), ValueError), (dict(genes=[0], value=float("inf")), ValueError),
                    (dict(genes=[0], rows_per_call=0), ValueError), (dict(genes=[0], tol=-1.0), ValueError),
                    (dict(genes=[0], rtol=1.0), TypeError)):
        with pytest.raises(exc, match="knockout_steady_states"):
            sys_.knockout_steady_states(x0, **kw)
    with pytest.raises(RuntimeError, match="no CPU path|must live on the GPU"):
        sys_.knockout_steady_states(x0, [0, 3])


def test_reached_is_the_graph_search_of_the_knockout_tests():
    from test_hillko_cpu import descendants
    sys_, _ = cpu_system(65)
    for g in range(65):
        assert np.array_equal(sys_.reached(g), descendants(sys_, g)), g


def test_steady_state_recovery_refuses_a_model_of_another_size_without_a_gpu():
    import phoenix_amd
    sys_, _ = cpu_system(12)
    net = phoenix_amd.ODENet("cpu", 16, neurons=4)
    with pytest.raises(ValueError, match="the model has 16 genes, the system 12"):
        phoenix_amd.steady_state_recovery(net, sys_, torch.zeros(2, 16), genes=[0])


# --------------------------------------------------------------------------- recovery statistics
def test_steady_state_recovery_scores_on_planted_arrays():
    import phoenix_amd
    from phoenix_amd.analysis import recovery_scores
    from phoenix_amd.steady import KnockoutSteadyStates, SteadyStates
    S = collections.namedtuple("S", ("y", "status"))
    rng = np.random.default_rng(5)
    K, B, N, genes = 3, 4, 5, [1, 0, 2]
    regulated = np.array([True, True, False, True, True])

    def screen(base, ko, bad_base=(), bad_ko=()):
        sb, sk = np.zeros(B, np.int32), np.zeros(K * B, np.int32)
        sb[list(bad_base)] = 1
        sk[list(bad_ko)] = 2
        return KnockoutSteadyStates(genes, S(base, sb), S(ko.reshape(K * B, N), sk), None, None)

    tb, lb = rng.random((B, N)), rng.random((B, N))
    td, ld = rng.standard_normal((K, B, N)), rng.standard_normal((K, B, N))
    td[1, :, 3] = 0.0                                   # a gene the held gene does not reach: a true 0, not counted
    true, learned = screen(tb, tb[None] + td), screen(lb, lb[None] + ld)
    s = phoenix_amd.steady_state_recovery_scores(genes, true, learned, regulated)
    want = phoenix_amd.knockout_recovery_scores(genes, td.mean(axis=1), ld.mean(axis=1))
    assert s.n_entries == want.n_entries == K * (N - 1) - 1 and s.n_unconverged == 0
    for a, b in zip(s[2:6], want[1:5]):
        assert np.isclose(a, b, rtol=1e-12, atol=0)
    assert np.isclose(s.base_pearson, np.corrcoef(tb[:, regulated].ravel(), lb[:, regulated].ravel())[0, 1], rtol=1e-12, atol=0)
    assert np.isclose(s.base_rms, np.sqrt(np.mean((tb[:, regulated] - lb[:, regulated]) ** 2)), rtol=1e-12, atol=0)
    others = np.ones((K, N), bool)
    others[np.arange(K), genes] = False
    mt, ml = (np.where(others, np.abs(d).mean(axis=1), 0).sum(axis=1) / 4 for d in (td, ld))
    assert np.isclose(s.scores_spearman, recovery_scores(mt, ml)[2], rtol=1e-12, atol=0)
    assert s.true is true and s.learned is learned and s.genes == genes
    # learned == true: 1 throughout and distance 0; tensors are taken as they come
    same = phoenix_amd.steady_state_recovery_scores(genes, true, screen(torch.from_numpy(tb), torch.from_numpy(tb[None] + td)))
    assert same[2:6] == pytest.approx((1.0, 1.0, 1.0, 1.0), rel=0, abs=1e-12)
    assert same.base_pearson == pytest.approx(1.0, abs=1e-12) and same.base_rms == 0.0
    assert same.scores_spearman == pytest.approx(1.0, abs=1e-12)
    # rows that did not converge on either side are left out of the means, and counted
    t2 = screen(tb, tb[None] + td, bad_base=[3], bad_ko=[0 * B + 1])
    l2 = screen(lb, lb[None] + ld, bad_ko=[2 * B + 0, 0 * B + 1])
    keep = np.ones((K, B), bool)
    keep[:, 3] = False
    keep[0, 1] = keep[2, 0] = False
    part = phoenix_amd.steady_state_recovery_scores(genes, t2, l2, regulated)
    mean = lambda d: np.stack([d[k][keep[k]].mean(axis=0) for k in range(K)])      # noqa: E731
    want = phoenix_amd.knockout_recovery_scores(genes, mean(td), mean(ld))
    assert part.n_unconverged == 3 and part.n_entries == want.n_entries
    for a, b in zip(part[2:6], want[1:5]):
        assert np.isclose(a, b, rtol=1e-12, atol=0)
    assert np.isclose(part.base_rms, np.sqrt(np.mean((tb[:3][:, regulated] - lb[:3][:, regulated]) ** 2)), rtol=1e-12, atol=0)
    # a knockout without a counted row is left out altogether
    gone = phoenix_amd.steady_state_recovery_scores(genes, screen(tb, tb[None] + td, bad_ko=range(B, 2 * B)), learned)
    assert gone.per_gene.n_entries.tolist()[1] == 0 and np.isfinite(gone.pearson) and np.isfinite(gone.scores_spearman)
    with pytest.raises(ValueError, match="steady_state_recovery_scores"):
        phoenix_amd.steady_state_recovery_scores([0, 1], true, learned)
