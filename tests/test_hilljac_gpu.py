"""phx_hill_jacobian (csrc/phx_hilljac.hip) and `analysis.jacobian_recovery` on the device.  Run with `-m gpu`.

Reference: J64 = `simulator.jacobian_reference` in float64 on the float32-rounded states, itself held to central differences
of the expression strings in tests/test_hilljac_cpu.py.  Bar on every value, by |device - J64| / max(1, |J64|): 5e-6, the
project's bar for the simulator's rates (tests/test_simulator_gpu.py); the float32 run of the reference on the host stays
within a quarter of it on the shipped network (tests/test_hilljac_cpu.py).  The reduced modes are held to the float64 mean
of J64 by the same bar, and to the float64 mean of the device's own mode-0 values by one float32 rounding.

Networks: the shipped 350-gene one (golden G11) and the synthetic ones of tests/test_simulator_cpu.py (the project's equation
builder, with the gene that fills the 24-slot stack and the gene with unary minus) in which two regulated genes are
rewritten by hand: one divides by an expression of a variable, one sums 40 activations.

Measured on an MI355X: 4.0e-7 on G11, 2.7e-7 ... 7.8e-7 on the synthetic networks (the worst entry belongs to the gene that
multiplies 24 activations), 1.1e-6 over the 70 000 rows, 2.7e-7 in the reduced modes."""
import functools

import numpy as np
import pytest
import torch

from test_hilljac_cpu import GPU_BAR, g11_states, g11_system, metric, rule_zeros
from test_simulator_cpu import CHAIN, compiled_depth, synthetic_network, synthetic_states

pytestmark = pytest.mark.gpu

WIDE = 40


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "these tests need the MI355X"
    return torch.device("cuda:0")


@functools.lru_cache(maxsize=None)
def network(N):
    """(names, expressions, info) of the synthetic N-gene network with the first two regulated genes rewritten: `divx`
    divides an activation by 1 + G^2 of another gene, `wide` is the mean of WIDE activations of distinct genes"""
    from phoenix_amd import simulator as sim
    names, exprs, info = synthetic_network(N)
    exprs, info = list(exprs), dict(info)
    rs = np.random.RandomState(7000 + N)
    free = [g for g in range(N - 2) if not info["is_input"][g]]
    divx, wide = free[0], free[1]
    a, b = (names[i] for i in rs.choice(N - 2, 2, replace=False))
    exprs[divx] = "(0.9 * fAct(%s, 0.3, 2.1) / (1 + %s * %s) - %s) / 1.5" % (a, b, b, names[divx])
    regs = rs.choice(N - 2, WIDE, replace=False)
    terms = []
    for i in regs:
        w, n, ec50 = rs.uniform(0.5, 1.0), rs.uniform(1.39, 3.0), rs.uniform(0.25, 0.5)
        assert sim.fact_constants(ec50, n)[1] > 0
        terms.append("%.9g * fAct(%s, %.9g, %.9g)" % (w, names[i], ec50, n))
    exprs[wide] = "((%s) / %d - %s) / 1" % (" + ".join(terms), WIDE, names[wide])
    info.update(divx=divx, wide=wide, wide_regs=np.sort(regs), div_by=names.index(b))
    assert compiled_depth(names, exprs[info["deep"]])[0] == sim.MAX_STACK == CHAIN
    return names, exprs, info


@functools.lru_cache(maxsize=None)
def system(N):
    from phoenix_amd.simulator import OPS, HillSystem
    names, exprs, info = network(N)
    sys_ = HillSystem(names, exprs, device="cuda:0")
    pat = sys_.jacobian_pattern()
    row = lambda g: pat.regulator[pat.ptr[g]:pat.ptr[g + 1]]                     # noqa: E731
    ops = lambda g: sys_.code_host[sys_.off_host[g]: sys_.off_host[g] + sys_.len_host[g], 0].tolist()   # noqa: E731
    assert set(info["wide_regs"].tolist()) <= set(row(info["wide"]).tolist()) and len(row(info["wide"])) >= WIDE
    assert info["div_by"] in row(info["divx"]) and ops(info["divx"]).count(OPS["DIV"]) == 2
    assert ops(info["unary"]).count(OPS["NEG"]) == 2 and ops(info["deep"]).count(OPS["FACT"]) == CHAIN
    assert np.all(np.diff(pat.ptr)[info["is_input"]] == 0)
    return sys_, info


def states(N, B, info, seed=0):
    """float32 states from (-0.2, 1.2) without (-1e-3, 1e-3); the regulators of the deep gene from (0.8, 1.2)"""
    x = synthetic_states(N, B, info, seed)
    x[np.abs(x) < 1e-3] = np.float32(2e-3)
    return x


def device_jacobian(sys_, x, reduce=None):
    jac = sys_.jacobian(torch.from_numpy(x).to(sys_.code.device), reduce)
    pat = sys_.jacobian_pattern()
    assert jac.value.dtype == torch.float32 and jac.regulator.dtype == jac.target.dtype == torch.int64
    assert np.array_equal(jac.regulator.cpu().numpy(), pat.regulator) and np.array_equal(jac.target.cpu().numpy(), pat.target)
    return jac.value.cpu().numpy()


def hold(tag, sys_, x, rows=None):
    """mode 0 at the states x against J64 (of the rows `rows` only, when given)"""
    from phoenix_amd.simulator import jacobian_reference
    got = device_jacobian(sys_, x)
    assert got.shape == (x.shape[0], len(sys_.jacobian_pattern().regulator))
    if rows is not None:
        got, x = got[rows], x[rows]
    J64 = jacobian_reference(sys_, x.astype(np.float64))
    err = metric(got, J64)
    b, e = np.unravel_index(int(err.argmax()), err.shape)
    print("%s: max |device - J64| / max(1, |J64|) = %.2e (state %d, entry %d -> %d); %d entries, max |J64| %.2f"
          % (tag, err.max(), b, sys_.jacobian_pattern().regulator[e], sys_.jacobian_pattern().target[e], err.shape[1],
             np.abs(J64).max()))
    assert np.all(np.isfinite(got)) and err.max() < GPU_BAR
    zero = rule_zeros(sys_, x)
    assert np.all(got[zero] == 0) and np.all(J64[zero] == 0) and zero.any()      # what the rules make 0 is 0
    return got, J64


# --------------------------------------------------------------------------- mode 0
def test_shipped_network(dev):
    from phoenix_amd.simulator import HillSystem
    host, names, eqns = g11_system()
    sys_ = HillSystem(names, eqns, device=dev)
    rs = np.random.RandomState(21)
    x = g11_states()
    zero = x[0].copy()
    zero[::3] = 0.0                                                              # exact zeros, regulators among them
    negative = rs.uniform(-0.2, -1e-3, 350).astype(np.float32)
    x = np.concatenate([x, zero[None], negative[None]])
    got, J64 = hold("G11 B=8", sys_, x)
    pat = sys_.jacobian_pattern()
    off = pat.regulator != pat.target
    assert np.all(got[7][off] == 0) and np.all(got[7][~off] < 0)                 # every activation is flat at TF < 0
    zreg = (zero == 0)[pat.regulator] & off
    assert np.all(got[6][zreg] == 0) and zreg.sum() > 100
    assert np.mean(got[:6] != 0) > 0.8
    # [B, 1, N] is the same call
    again = sys_.jacobian(torch.from_numpy(x).to(dev).reshape(8, 1, 350)).value.cpu().numpy()
    assert np.array_equal(again, got)


@pytest.mark.parametrize("N", [63, 64, 65, 1025])
def test_synthetic_networks(dev, N):
    """one wave minus / exactly / plus one gene and more than four workgroups of entries; the deep, unary, dividing and
    40-regulator genes are in every one of them"""
    sys_, info = system(N)
    x = states(N, 5, info)
    assert np.any(x < 0) and np.any(x > 1) and np.all(np.abs(x) >= 1e-3)
    got, J64 = hold("N=%d B=5" % N, sys_, x)
    pat = sys_.jacobian_pattern()
    for g in ("deep", "unary", "divx", "wide"):
        sl = slice(pat.ptr[info[g]], pat.ptr[info[g] + 1])
        err = metric(got[:, sl], J64[:, sl]).max()
        print("  %-5s gene: %2d entries, max |J64| %.3f, err %.2e" % (g, sl.stop - sl.start, np.abs(J64[:, sl]).max(), err))
        assert np.count_nonzero(J64[:, sl]) > 0.4 * J64[:, sl].size              # the gene tests something
    if N == 1025:
        assert got.shape[1] > 4 * 256


def test_more_rows_than_a_grid_dimension(dev):
    """B = 70 000 > 65 535 rows over the capped gridDim.y: a seeded sample of 2 000 rows and the two ends"""
    sys_, info = system(64)
    x = states(64, 70000, info)
    rows = np.unique(np.concatenate([[0, 69999], np.random.RandomState(70).choice(70000, 2000, replace=False)]))
    hold("N=64 B=70000", sys_, x, rows=rows)


def test_a_regulator_the_program_never_pushes_is_plus_zero(dev):
    """the raw call with a pattern of the caller's own: -(a * a) * 1.5 has no b; the rules alone would leave -0"""
    from phoenix_amd import _lib, engine
    from phoenix_amd.simulator import HillSystem
    sys_ = HillSystem(["a", "b", "y"], ["input gene", "input gene", "-(a * a) * 1.5"], device=dev)
    x = torch.tensor([[0.3, 0.7, 0.2], [-0.4, 0.1, 0.9], [0.0, -0.3, 0.5]], device=dev)
    eptr = torch.tensor([0, 0, 0, 2], dtype=torch.int64, device=dev)
    ereg = torch.tensor([0, 1], dtype=torch.int32, device=dev)
    out = torch.full((3, 2), float("nan"), device=dev)
    rc = _lib.load().phx_hill_jacobian(*sys_._args(), engine._p(eptr), engine._p(ereg), engine._p(x), 3, 3, 2, 0, engine._p(out),
                                       None, 0, engine._stream_ptr())
    assert rc == 0
    out = out.cpu().numpy()
    a = x[:, 0].cpu().numpy()
    assert np.array_equal(out[:, 0], -(a + a) * np.float32(1.5)) and np.all(out[:, 1] == 0) and not np.any(np.signbit(out[:, 1]))


# --------------------------------------------------------------------------- modes 1 and 2
@pytest.mark.parametrize("B", [1, 2, 257, 4099])
def test_reduced_modes(dev, B):
    """one chunk (B = 1, 2: no workspace), 9 chunks of unequal length and 129 chunks"""
    from phoenix_amd import _lib
    from phoenix_amd.simulator import jacobian_reference
    sys_, info = system(64)
    x = states(64, B, info, seed=B)
    J64 = jacobian_reference(sys_, x.astype(np.float64))
    full = device_jacobian(sys_, x).astype(np.float64)
    E = J64.shape[1]
    assert _lib.load().phx_hill_jacobian_workspace_bytes(B, 64, E, 1) == (0 if B <= 32 else -(-B // 32) * E * 8)
    got = {}
    for reduce, ref, own in (("mean", J64.mean(axis=0), full.mean(axis=0)),
                             ("mean_abs", np.abs(J64).mean(axis=0), np.abs(full).mean(axis=0))):
        got[reduce] = device_jacobian(sys_, x, reduce)
        assert got[reduce].shape == (E,)
        err = metric(got[reduce], ref)
        # float64 sums of the device's own values, in any order, agree to B 2^-52 of the mean magnitude; then one rounding
        slack = np.spacing(np.abs(got[reduce])).astype(np.float64) + B * 2.0 ** -52 * np.abs(full).mean(axis=0)
        print("B=%d %s: against the fp64 mean of J64 %.2e; against the fp64 mean of mode 0, in roundings: %.2f"
              % (B, reduce, err.max(), np.max(np.abs(got[reduce] - own) / slack)))
        assert err.max() < GPU_BAR
        assert np.all(np.abs(got[reduce] - own) <= slack)
        assert np.array_equal(device_jacobian(sys_, x, reduce), got[reduce])     # bit for bit
    assert np.all(got["mean_abs"] >= np.abs(got["mean"]) * (1 - 2.0 ** -23))
    if B == 1:
        assert np.array_equal(got["mean"], full[0].astype(np.float32)) and np.array_equal(got["mean_abs"], np.abs(got["mean"]))


# --------------------------------------------------------------------------- the recovery score
def test_jacobian_recovery(dev):
    import phoenix_amd
    sys_, info = system(64)
    torch.manual_seed(64)
    net = phoenix_amd.ODENet(dev, 64, neurons=8)
    with torch.no_grad():
        for lin in (net.net_sums.linear_out, net.net_prods.linear_out, net.net_alpha_combine.linear_out):
            lin.weight.normal_(0.0, 0.3)
    x = torch.from_numpy(states(64, 37, info, seed=5)).to(dev)
    pat = sys_.jacobian_pattern()
    matrix = phoenix_amd.jacobian_matrix(net, x, reduce="mean")
    value = sys_.jacobian(x, "mean").value
    results = {}
    for diagonal in (False, True):
        keep = np.flatnonzero(np.ones(len(pat.regulator), bool) if diagonal else pat.regulator != pat.target)
        r = results[diagonal] = phoenix_amd.jacobian_recovery(net, sys_, x.reshape(37, 1, 64) if diagonal else x, diagonal=diagonal)
        assert isinstance(r, phoenix_amd.JacobianRecovery) and r.n_edges == len(keep)
        assert np.array_equal(r.regulator.cpu().numpy(), pat.regulator[keep]) and r.regulator.dtype == torch.int64
        assert np.array_equal(r.target.cpu().numpy(), pat.target[keep]) and r.target.dtype == torch.int64
        assert r.learned.dtype == r.true.dtype == torch.float32 and r.learned.is_cuda and r.true.is_cuda
        assert torch.equal(r.learned, matrix[r.regulator, r.target])             # bit for bit
        assert torch.equal(r.true, value[torch.from_numpy(keep).to(dev)])
        scores = phoenix_amd.recovery_scores(r.true.cpu().numpy(), r.learned.cpu().numpy())
        np.testing.assert_array_equal(np.array([r.sign_agreement, r.pearson, r.spearman, r.slope]), np.array(scores))
        assert all(np.isfinite(s) for s in scores) and 0 <= r.sign_agreement <= 1 and abs(r.pearson) <= 1
        print("diagonal=%s: %d edges, sign agreement %.3f, pearson %.3f, spearman %.3f, slope %.3f"
              % ((diagonal, r.n_edges) + scores))
    n_diag = int((pat.regulator == pat.target).sum())
    assert results[True].n_edges == results[False].n_edges + n_diag == len(pat.regulator) and n_diag == int((~info["is_input"]).sum())
    with pytest.raises(ValueError, match="y must be"):
        phoenix_amd.jacobian_recovery(net, sys_, x[:, :63])


def test_a_system_of_input_genes_has_an_empty_jacobian(dev):
    from phoenix_amd import engine
    from phoenix_amd.simulator import HillSystem
    sys_ = HillSystem(["A", "B", "C"], ["input gene"] * 3, device=dev)
    pat = sys_.jacobian_pattern()
    assert pat.regulator.shape == pat.target.shape == (0,) and pat.ptr.tolist() == [0, 0, 0, 0]
    before = {k: v.data_ptr() for k, v in engine._ws_cache.items()}
    x = torch.rand(40, 3, device=dev)
    for reduce, shape in ((None, (40, 0)), ("mean", (0,)), ("mean_abs", (0,))):
        jac = sys_.jacobian(x, reduce)
        assert tuple(jac.value.shape) == shape and jac.value.is_cuda and jac.value.dtype == torch.float32
        assert jac.regulator.numel() == jac.target.numel() == 0 and jac.regulator.dtype == torch.int64
    assert {k: v.data_ptr() for k, v in engine._ws_cache.items()} == before      # not even a workspace was asked for
