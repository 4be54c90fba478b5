"""k_hill_knockouts (csrc/phx_hillko.hip; `HillSystem.knockouts`, `HillSystem.knockout_effects`, `knockout_recovery`) on
the synthetic networks of tests/test_simulator_cpu.py against `knockouts_reference` in float64 (held to the oracle and to
a case worked by hand in tests/test_hillko_cpu.py).  Run with `-m gpu`.

Bars: TRAJ_BAR = 1e-5 max-norm relative on trajectories, per call and per gene -- the bar tests/test_simulator_gpu.py holds
phx_hill_simulate to; the arithmetic of a row is that kernel's.  On shift and magnitude 2 TRAJ_BAR scale absolute: every
trajectory entry is within TRAJ_BAR scale, a difference of two within twice that, and so is a mean of such differences.
Everything structural is bitwise: the held column, out[0], input genes, the genes a held gene does not reach, and a call
against itself in another group."""
import functools

import numpy as np
import pytest
import torch

from test_hillko_cpu import DT_MAX, TIMES, descendants, gene_without_descendants, untouched
from test_knockout_cpu import reference64
from test_simulator_cpu import synthetic_network, synthetic_states

pytestmark = pytest.mark.gpu

TRAJ_BAR = 1e-5                                   # tests/test_simulator_gpu.py


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "these tests need the MI355X"
    return torch.device("cuda:0")


@functools.lru_cache(maxsize=None)
def system(N):
    from phoenix_amd.simulator import HillSystem
    names, exprs, info = synthetic_network(N)
    return HillSystem(names, exprs, device="cuda:0"), info


def reference(sys_, x0, times, genes, values, dt_max=DT_MAX):
    from phoenix_amd.simulator import knockouts_reference
    ref = knockouts_reference(sys_, x0, times, genes, values, dt_max)
    assert ref.dtype == np.float64 and np.all(np.isfinite(ref))
    return ref


def run(sys_, x0, times, genes, values, dt_max=DT_MAX):
    got = sys_.knockouts(torch.from_numpy(x0).to(sys_.device), times, genes, values, dt_max)
    assert got.dtype == torch.float32 and tuple(got.shape) == (len(times), len(genes), x0.shape[0], sys_.N)
    return got.cpu().numpy()


def hold(tag, got, ref):
    """TRAJ_BAR max-norm relative, per call and per gene"""
    assert got.shape == ref.shape
    scale = float(np.max(np.abs(ref)))
    err = np.abs(got.astype(np.float64) - ref).max(axis=(0, 2))      # [K, N]: over all times and samples
    k, n = np.unravel_index(int(err.argmax()), err.shape)
    print("%s: max err / max|ref| %.2e (call %d, gene %d); max|ref| %.3f" % (tag, err.max() / scale, k, n, scale))
    assert np.all(err <= TRAJ_BAR * scale), (tag, int(k), int(n), float(err.max() / scale))
    return scale


def screen_calls(sys_, info):
    """the K = 7 calls of the screen cases: the unperturbed system, an input gene (at a negative level: its targets see fAct
    at TF <= 0), the deep and the unary gene (the last gene of the network), a gene nothing depends on, and gene 0 twice"""
    inputs = np.flatnonzero(info["is_input"]).tolist()
    inp = next((g for g in inputs if descendants(sys_, g).any()), inputs[0])      # one that regulates something, if any does
    lone = gene_without_descendants(sys_)
    return [-1, inp, info["deep"], info["unary"], 0, lone, 0], [0.0, -0.15, 0.0, 0.4, 0.0, 0.9, 1.7]


@functools.lru_cache(maxsize=None)
def screen_case(N):
    """(system, info, x0, genes, values, reference, result) of the screen case at N genes: computed once, shared, read only"""
    sys_, info = system(N)
    if N == 8192:       # the largest network: 8 genes per thread, the largest LDS footprint
        B, times = 1, TIMES[:3]
        genes, values = [-1, info["unary"], 0], [0.0, -0.15, 1.7]
    else:
        B, times = 3, TIMES
        genes, values = screen_calls(sys_, info)
    x0 = synthetic_states(N, B, info, seed=4)
    ref = reference(sys_, x0, times, genes, values)
    got = run(sys_, x0, times, genes, values)
    for a in (x0, ref, got):
        a.setflags(write=False)
    return sys_, info, x0, genes, values, ref, got


@pytest.mark.parametrize("N", [63, 65, 1025, 8192])
def test_knockouts_against_float64(dev, N):
    """one wave minus / plus one gene; 1025: two genes per thread with the guard in the middle of a thread's list and gene
    1024 held; 8192: eight genes per thread"""
    sys_, info, x0, genes, values, ref, got = screen_case(N)
    assert any(v < 0 for v in values) and info["unary"] == N - 1 and info["unary"] in genes
    hold("N=%d K=%d" % (N, len(genes)), got, ref)


@pytest.mark.parametrize("N", [63, 65, 1025, 8192])
def test_knockouts_structure_is_bitwise(dev, N):
    sys_, info, x0, genes, values, ref, got = screen_case(N)
    scale = float(np.max(np.abs(ref)))
    moved_most = 0.0
    for k, (g, v) in enumerate(zip(genes, values)):
        want0 = x0.copy()
        if g >= 0:
            want0[:, g] = v
            assert np.all(got[:, k, :, g] == np.float32(v)), (k, g)            # the held column, at every time
        assert np.array_equal(got[0, k], want0), k                              # out[0]: x0 with that column replaced
        free = sys_.is_input.copy()
        if g >= 0:
            free[g] = False
        assert np.all(got[:, k][:, :, free] == want0[None][:, :, free]), k      # input genes are constant
        keep = untouched(sys_, g)
        assert np.array_equal(got[:, k][:, :, keep], got[:, 0][:, :, keep]), (k, g)      # what g does not reach: the -1 call
        if g >= 0:
            reach = descendants(sys_, g) & (np.arange(N) != g)
            moved = float(np.abs(ref[:, k] - ref[:, 0])[:, :, reach].max()) if reach.any() else 0.0
            print("call %d, gene %d at %.2f: %d genes reached, %d not; the reference moves a reached gene by %.2e of max|ref|"
                  % (k, g, v, reach.sum(), keep.sum(), moved / scale))
            moved_most = max(moved_most, moved)
    assert genes[0] == -1 and moved_most > 100 * TRAJ_BAR * scale      # not vacuous: some reached gene does move


def test_a_call_does_not_depend_on_its_group(dev):
    """K = 9: full groups and a remainder at every supported group size; a gene beside a duplicate of itself and beside
    the same gene at another level; each call alone (K = 1: one live slot) and all of them in reversed order"""
    sys_, info = system(65)
    x0 = synthetic_states(65, 3, info, seed=4)
    genes = [info["deep"], info["deep"], -1, 0, 0, info["unary"], 7, int(np.flatnonzero(info["is_input"])[0]), 33]
    values = [0.0, 0.0, 0.0, 0.0, 1.7, 0.4, -0.15, 0.6, 1.1]
    got = run(sys_, x0, TIMES, genes, values)
    assert np.array_equal(got[:, 0], got[:, 1]) and not np.array_equal(got[:, 3], got[:, 4])
    back = run(sys_, x0, TIMES, genes[::-1], values[::-1])
    assert np.array_equal(back[:, ::-1], got)
    for k in range(9):
        alone = run(sys_, x0, TIMES, genes[k:k + 1], values[k:k + 1])
        assert np.array_equal(alone[:, 0], got[:, k]), k


def test_knockouts_backwards_in_time(dev):
    sys_, info = system(65)
    x0, times = synthetic_states(65, 3, info, seed=3), [1.0, 0.6, 0.0]
    genes, values = [-1, info["unary"], 0], [0.0, 0.4, 1.7]
    hold("N=65 decreasing", run(sys_, x0, times, genes, values), reference(sys_, x0, times, genes, values))


def test_knockouts_at_a_single_time(dev):
    """T = 1: no interval, the output is the modified x0"""
    sys_, info = system(65)
    x0 = synthetic_states(65, 3, info, seed=1)
    genes, values = [-1, info["unary"], 0], [0.0, 0.4, 1.7]
    got, ref = run(sys_, x0, [0.7], genes, values), reference(sys_, x0, [0.7], genes, values)
    assert got.shape == (1, 3, 3, 65)
    hold("N=65 T=1", got, ref)
    assert np.array_equal(got[0, 0], x0) and np.all(got[0, 2, :, 0] == np.float32(1.7))
    assert np.array_equal(got[0, 2, :, 1:], x0[:, 1:]) and np.array_equal(got[0, 1, :, :64], x0[:, :64])
    assert np.all(got[0, 1, :, 64] == np.float32(0.4))


def test_knockouts_of_a_single_sample(dev):
    sys_, info = system(65)
    x0, times = synthetic_states(65, 1, info, seed=2), [0.0, 0.25, 0.3]
    genes, values = [0, -1, info["deep"], info["unary"], 0], [1.7, 0.0, 0.0, 0.4, 0.0]
    hold("N=65 B=1", run(sys_, x0, times, genes, values), reference(sys_, x0, times, genes, values))


def test_knockout_effects_of_the_simulator(dev):
    """`HillSystem.knockout_effects` in blocks of 2 genes and in one block against the scoring formulas in float64 on the
    float64 trajectories"""
    sys_, info, x0, genes, values, ref, _ = screen_case(65)
    G = len(genes) - 1                                   # the screen's calls after the -1 call, a gene twice included
    r_scores, r_shift, r_mag = reference64(ref[:, 0], ref[:, 1:].reshape(len(TIMES), G * 3, 65), genes[1:])
    scale = float(np.max(np.abs(ref)))
    x0d = torch.from_numpy(x0.copy()).to(sys_.device)
    for per_launch in (2, 64):
        eff = sys_.knockout_effects(x0d, genes[1:], values[1:], TIMES, DT_MAX, genes_per_launch=per_launch)
        assert eff.genes == genes[1:] and eff.scores.dtype == np.float32 and tuple(eff.shift.shape) == (G, 65)
        shift, mag = eff.shift.cpu().numpy(), eff.magnitude.cpu().numpy()
        e_shift, e_mag = np.abs(shift - r_shift).max(), np.abs(mag - r_mag).max()
        e_scores = np.abs(eff.scores - r_scores).max()
        print("genes_per_launch %d: shift err %.2e, magnitude err %.2e, scores err %.2e; bar %.2e"
              % (per_launch, e_shift, e_mag, e_scores, 2 * TRAJ_BAR * scale))
        assert e_shift <= 2 * TRAJ_BAR * scale and e_mag <= 2 * TRAJ_BAR * scale and e_scores <= 2 * TRAJ_BAR * scale
        for i, g in enumerate(genes[1:]):
            keep = untouched(sys_, g)
            assert np.all(shift[i, keep] == 0) and np.all(mag[i, keep] == 0), (i, g)       # exactly
            if not descendants(sys_, g).any():
                assert eff.scores[i] == 0, (i, g)
        assert any(not descendants(sys_, g).any() for g in genes[1:]) and np.any(eff.scores > 0)
        only = sys_.knockout_effects(x0d, genes[1:], values[1:], TIMES, DT_MAX, genes_per_launch=per_launch, want_matrices=False)
        assert only.shift is None and only.magnitude is None and np.array_equal(only.scores, eff.scores)


def test_knockout_recovery_end_to_end(dev):
    """a random model against the simulator: `true` and `learned` are the two screens called directly, bit for bit, and the
    statistics are `knockout_recovery_scores` of them; nothing is asked of a random model's quality"""
    import phoenix_amd
    from phoenix_amd.analysis import _average_ranks, _pearson
    N, B = 96, 5
    sys_, info = system(N)
    torch.manual_seed(0)
    net = phoenix_amd.ODENet(dev, N, neurons=8)
    y0 = torch.from_numpy(synthetic_states(N, B, info, seed=4)).to(dev)
    genes, values = [0, info["deep"], info["unary"], gene_without_descendants(sys_)], [0.0, 1.7, 0.4, 0.0]
    t = torch.from_numpy(np.arange(0, 1, 0.25))
    rec = phoenix_amd.knockout_recovery(net, sys_, y0, genes, values, t, dt_max=0.05, min_effect=1e-6)
    learned = phoenix_amd.knockout_effects(net, y0, genes, values, t)
    true = sys_.knockout_effects(y0, genes, values, t, 0.05)
    assert rec.genes == genes == rec.true.genes == rec.learned.genes
    for a, b in ((rec.true, true), (rec.learned, learned)):
        assert np.array_equal(a.scores, b.scores) and torch.equal(a.shift, b.shift) and torch.equal(a.magnitude, b.magnitude)
    s = phoenix_amd.knockout_recovery_scores(genes, true.shift, learned.shift, min_effect=1e-6)
    same = lambda a, b: a == b or (np.isnan(a) and np.isnan(b))      # noqa: E731
    assert rec.n_entries == s.n_entries > 0
    assert all(same(a, b) for a, b in zip(rec[2:6], s[1:5]))
    assert all(np.array_equal(a, b, equal_nan=True) for a, b in zip(rec.per_gene, s.per_gene))
    assert rec.per_gene.n_entries[3] == 0 and rec.per_gene.n_entries[0] > 0
    want = _pearson(_average_ranks(true.scores.astype(np.float64)), _average_ranks(learned.scores.astype(np.float64)))
    assert same(rec.scores_spearman, want) and -1.0 <= rec.scores_spearman <= 1.0
    print("knockout_recovery of a random model: %d entries, sign %.3f pearson %.3f spearman %.3f slope %.3g, scores %.3f"
          % (rec.n_entries, rec.sign_agreement, rec.pearson, rec.spearman, rec.slope, rec.scores_spearman))
