"""The fused gene-influence scan on the MI355X: phx_influence_scores (through the C ABI, via phoenix_amd.engine) against
float64 evaluations of the same formula on the same tensors, `gene_influence_scores(fused=True)` against the reference's
own scores (golden G10), and `gene_influence_matrix` against the eager path and against `odeint_calls`' own output.

The bar everywhere is the one test_gpu_parity.py::test_f3_gene_influence_scores holds the eager path to: 2e-5 relative.
Every test prints the figures it measured before it asserts (run with -s to see them).
Measured on an MI355X (test_kernel_against_float64, max relative error against float64):
    (T, pairs, B, N)        scores     worst targets entry
    (10, 8, 60, 11165)      6.8e-8     2.9e-7
    (10, 1, 60, 350)        1.8e-8     2.2e-7
    (2, 3, 7, 97)           9.5e-8     1.6e-7
    (10, 2, 24, 14691)      1.7e-8     2.8e-7
    (5, 40, 5, 96)          8.8e-8     3.0e-7
    (10, 4, 1, 33)          1.0e-7     1.6e-7
G10 through fused=True: 1.74e-5.  End to end: scores
against the eager path 1.4e-7 (dopri5, N = 350) and 6.4e-7 (rk4, N = 700), matrix against float64 1.6e-7 worst entry;
genes_per_launch 1, 2 and 8 gave identical bits.  Memory test: fused 25 349 632 bytes, eager 50 699 776, budget
25 408 000."""
import numpy as np
import pytest
import torch

from conftest import load_golden, relerr, sub
from test_gpu_parity import make_net, rand_params

pytestmark = pytest.mark.gpu

TOL = 2e-5      # test_f3_gene_influence_scores' bar


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "these tests need the MI355X"
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def pa():
    import phoenix_amd
    return phoenix_amd


def decades(shape, dev, seed):
    """positive values spread over four decades, so that the |differences| are too"""
    g = torch.Generator(device=dev).manual_seed(seed)
    x = torch.rand(shape, device=dev, generator=g)
    e = torch.rand(shape, device=dev, generator=g)
    return x * torch.pow(10.0, e * 4 - 3)


def reference64(sol, pairs, B, genes):
    """the formula of include/phoenix_hip.h in float64, pair by pair: (scores [pairs], targets [pairs, N])"""
    T, _, N = sol.shape
    tg = torch.empty((pairs, N), dtype=torch.float64, device=sol.device)
    sc = torch.empty(pairs, dtype=torch.float64, device=sol.device)
    for j in range(pairs):
        u = sol[1:, 2 * j * B:(2 * j + 1) * B].double()
        p = sol[1:, (2 * j + 1) * B:(2 * j + 2) * B].double()
        s = (u - p).abs().sum(dim=(0, 1))
        keep = torch.ones(N, dtype=torch.bool, device=sol.device)
        keep[genes[j]] = False
        tg[j] = s / ((T - 1) * B)
        sc[j] = s[keep].sum() / ((T - 1) * B * (N - 1))
    return sc, tg


def max_rel(got, ref):
    """largest |got - ref| / |ref| over the entries; an entry whose reference is exactly 0 (a target gene the perturbed
    gene does not reach) must be exactly 0"""
    err = (got.double() - ref).abs()
    zero = ref == 0
    assert not bool((err[zero] != 0).any())
    return float((err[~zero] / ref[~zero].abs()).max())


# --------------------------------------------------------------------------- 1. the reference's own scores
def test_fused_scores_match_the_reference(pa, dev):
    """golden G10 (`infl/`: the reference's scores from recorded draws, N = 24, n = 8) through fused=True, at the bar of
    test_f3_gene_influence_scores"""
    g = sub(load_golden("g10_analysis"), "infl/")
    net = make_net(pa, dev, sub(g, "p_"))
    inits, perts = torch.from_numpy(g["inits"]), torch.from_numpy(g["perts"])
    got = pa.gene_influence_scores(net, 24, "dopri5", n_random_inputs_per_gene=8, device=dev,
                                   draws=lambda k: (inits[k], perts[k]), fused=True)
    assert got.shape == g["scores"].shape and got.dtype == np.float32
    err = np.max(np.abs(got - g["scores"]) / np.abs(g["scores"]))
    print("G10 fused scores: max relative error %.3e" % err)
    assert err < TOL
    # default draws: runs end to end, positive finite scores, one per requested gene
    some = pa.gene_influence_scores(net, 24, "dopri5", n_random_inputs_per_gene=8, device=dev, genes=[3, 7], fused=True)
    assert some.shape == (2,) and np.all(np.isfinite(some)) and np.all(some > 0)


# --------------------------------------------------------------------------- 2. the kernel alone
@pytest.mark.parametrize("T,pairs,B,N", [(10, 8, 60, 11165), (10, 1, 60, 350), (2, 3, 7, 97), (10, 2, 24, 14691),
                                         (5, 40, 5, 96), (10, 4, 1, 33)])
def test_kernel_against_float64(pa, dev, T, pairs, B, N):
    from phoenix_amd import engine
    sol = decades((T, 2 * pairs * B, N), dev, seed=N + pairs)
    genes = [int(g) for g in np.random.RandomState(N).randint(0, N, pairs)]
    genes[0], genes[-1] = N - 1, (0 if pairs > 1 else N - 1)      # the first and the last column are somebody's gene
    ref_s, ref_t = reference64(sol, pairs, B, genes)
    scores, targets = engine.influence_scores(sol, pairs, B, genes, want_targets=True)
    assert scores.shape == (pairs,) and targets.shape == (pairs, N)
    e_s, e_t = max_rel(scores, ref_s), max_rel(targets, ref_t)
    print("kernel vs float64 (T=%d pairs=%d B=%d N=%d): scores %.3e  targets (worst entry) %.3e" % (T, pairs, B, N, e_s, e_t))
    assert e_s < TOL
    assert e_t < TOL
    # the score is the mean of its row of targets over every gene but the perturbed one
    t64 = targets.double()
    for j in range(pairs):
        mean = (t64[j].sum() - t64[j, genes[j]]) / (N - 1)
        assert abs(float(mean) - float(scores[j])) <= TOL * float(scores[j]), j
    # without targets (s in the workspace): the same scores, bit for bit; and again on the same tensor
    alone, none = engine.influence_scores(sol, pairs, B, genes, want_targets=False)
    assert none is None and torch.equal(alone, scores)
    scores2, targets2 = engine.influence_scores(sol, pairs, B, genes, want_targets=True)
    assert torch.equal(scores2, scores) and torch.equal(targets2, targets)
    # the initial states (output 0) are not part of any sum
    sol[0] = float("nan")
    scores3, targets3 = engine.influence_scores(sol, pairs, B, genes, want_targets=True)
    assert torch.equal(scores3, scores) and torch.equal(targets3, targets)


# --------------------------------------------------------------------------- 3. the perturbed gene is skipped by index
@pytest.mark.parametrize("T,pairs,B,N", [(10, 3, 60, 350), (10, 2, 7, 11165)])
def test_perturbed_column_is_skipped_not_subtracted(pa, dev, T, pairs, B, N):
    """the perturbed gene's own column differs by 1e6, every other by about 1e-3: `total - column` in float32 loses the
    score altogether (at N = 350 the own column sums to 5.4e8, where float32 steps by 32 or 64, and all the other
    columns together to about 94), so only a sum that never takes the column in matches float64"""
    from phoenix_amd import engine
    g = torch.Generator(device=dev).manual_seed(7)
    genes = [0, N - 1, N // 2][:pairs]
    sol = torch.rand((T, 2 * pairs * B, N), device=dev, generator=g)
    for j in range(pairs):
        u = sol[:, 2 * j * B:(2 * j + 1) * B]
        p = sol[:, (2 * j + 1) * B:(2 * j + 2) * B]
        p.copy_(u + 1e-3 * torch.rand(u.shape, device=dev, generator=g))
        p[:, :, genes[j]] = u[:, :, genes[j]] + 1e6
    ref_s, ref_t = reference64(sol, pairs, B, genes)
    scores, targets = engine.influence_scores(sol, pairs, B, genes, want_targets=True)
    e_s = max_rel(scores, ref_s)
    print("skip by index (N=%d): scores %.3e; diagonal entries %s" % (N, e_s, [float(targets[j, genes[j]]) for j in range(pairs)]))
    assert e_s < TOL
    assert max_rel(targets, ref_t) < TOL
    for j in range(pairs):        # reported as computed
        assert abs(float(targets[j, genes[j]]) - 1e6) < 1.0


# --------------------------------------------------------------------------- 4. end to end
def _draws(N, n, genes, seed):
    rs = np.random.RandomState(seed)
    d = {k: (torch.from_numpy(rs.rand(n, 1, N).astype(np.float32) - 0.5), torch.from_numpy(rs.rand(n).astype(np.float32) - 0.5))
         for k in genes}
    return lambda k: d[k]


def _matrix64(pa, net, N, n, genes, draws, t, method):
    """float64 evaluation of the matrix on `odeint_calls`' own output, all genes in one batch of calls"""
    inits = []
    for k in genes:
        a, col = (x.to(t.device) for x in draws(k))
        b = a.clone()
        b[:, 0, k] = col
        inits += [a, b]
    out = pa.odeint_calls(net, torch.stack(inits), t, method=method).double()     # [2G, T, n, 1, N]
    return torch.stack([(out[2 * i, 1:] - out[2 * i + 1, 1:]).abs().mean(dim=(0, 1, 2)) for i in range(len(genes))])


@pytest.mark.parametrize("N,H,n,method", [(350, 30, 7, "dopri5"), (700, 20, 7, "rk4")])
def test_matrix_end_to_end(pa, dev, N, H, n, method):
    genes = [0, 17, 349]
    net = make_net(pa, dev, rand_params(N, H, seed=N + H, std=0.6 / np.sqrt(N)))
    draws = _draws(N, n, genes, seed=N)
    t = torch.from_numpy(np.arange(0, 1, 0.1)).to(dev)
    ref_m = _matrix64(pa, net, N, n, genes, draws, t, method)
    results = {}
    for gpl in (1, 2, 8):
        scores, matrix = pa.gene_influence_matrix(net, N, method, n_random_inputs_per_gene=n, device=dev, genes=genes,
                                                  draws=draws, genes_per_launch=gpl)
        assert isinstance(scores, np.ndarray) and scores.shape == (3,) and scores.dtype == np.float32
        assert matrix.shape == (3, N) and matrix.is_cuda and matrix.dtype == torch.float32
        eager = pa.gene_influence_scores(net, N, method, n_random_inputs_per_gene=n, device=dev, genes=genes, draws=draws,
                                         genes_per_launch=gpl, fused=False)
        fused = pa.gene_influence_scores(net, N, method, n_random_inputs_per_gene=n, device=dev, genes=genes, draws=draws,
                                         genes_per_launch=gpl, fused=True)
        assert np.array_equal(fused, scores)               # the same scan without the matrix
        e_sc = float(np.max(np.abs(scores - eager) / np.abs(eager)))
        e_m = relerr(matrix.cpu().numpy(), ref_m.cpu().numpy())
        e_entry = max_rel(matrix, ref_m)
        print("%s N=%d genes_per_launch=%d: scores vs eager %.3e, matrix vs float64 %.3e (worst entry %.3e)"
              % (method, N, gpl, e_sc, e_m, e_entry))
        assert e_sc < TOL
        # (max-norm, the convention of every trajectory comparison here: launches that batch the calls differently
        # agree to the trajectory tolerance relative to the trajectory's scale, not entry by entry)
        assert e_m < TOL
        if gpl == 8:      # the very launch `_matrix64` made: what is left is the kernel's own summation, entry by entry
            assert e_entry < TOL
        for i, k in enumerate(genes):     # the score is the row mean without the perturbed gene's own entry
            row = matrix[i].double()
            assert abs(float((row.sum() - row[k]) / (N - 1)) - float(scores[i])) <= TOL * float(scores[i])
        results[gpl] = (scores, matrix.cpu().numpy())
    for gpl in (1, 2):
        e_sc = float(np.max(np.abs(results[gpl][0] - results[8][0]) / np.abs(results[8][0])))
        e_m = relerr(results[gpl][1], results[8][1])
        print("%s N=%d genes_per_launch %d vs 8: scores %.3e matrix %.3e" % (method, N, gpl, e_sc, e_m))
        assert e_sc < TOL and e_m < TOL


def test_default_draws_follow_the_eager_path(pa, dev):
    """without `draws` the fused scan consumes the generator exactly like the eager one: one seed, one set of scores"""
    N, n, genes = 350, 7, [3, 349, 0, 120, 77]
    net = make_net(pa, dev, rand_params(N, 30, seed=11, std=0.6 / np.sqrt(N)))
    kw = dict(n_random_inputs_per_gene=n, device=dev, genes=genes, genes_per_launch=2)
    torch.manual_seed(5)
    eager = pa.gene_influence_scores(net, N, "dopri5", **kw)
    torch.manual_seed(5)
    fused = pa.gene_influence_scores(net, N, "dopri5", fused=True, **kw)
    torch.manual_seed(5)
    scores, matrix = pa.gene_influence_matrix(net, N, "dopri5", **kw)
    err = float(np.max(np.abs(fused - eager) / np.abs(eager)))
    print("default draws, seed 5: fused vs eager scores %.3e" % err)
    assert err < TOL
    assert np.array_equal(scores, fused) and matrix.shape == (5, N)


# --------------------------------------------------------------------------- 5. non-finite inputs
def test_nan_propagates_to_its_pair_only(pa, dev):
    from phoenix_amd import engine
    T, pairs, B, N = 10, 4, 60, 350
    genes = [5, 9, 0, 349]
    sol = decades((T, 2 * pairs * B, N), dev, seed=3)
    clean_s, clean_t = engine.influence_scores(sol, pairs, B, genes, want_targets=True)
    sol[4, 3 * B + 11, 123] = float("nan")          # a perturbed row of pair 1, a column that is not its gene
    scores, targets = engine.influence_scores(sol, pairs, B, genes, want_targets=True)
    assert torch.isnan(scores[1]) and torch.isnan(targets[1, 123])
    assert int(torch.isnan(targets).sum()) == 1
    others = [0, 2, 3]
    assert torch.equal(scores[others], clean_s[others]) and torch.equal(targets[others], clean_t[others])
    # ... and in the perturbed gene's own column it reaches the matrix, not the score
    sol[4, 3 * B + 11, 123] = 1.0
    sol[2, 2 * B + 1, genes[1]] = float("inf")
    scores, targets = engine.influence_scores(sol, pairs, B, genes, want_targets=True)
    assert bool(torch.isfinite(scores).all()) and not bool(torch.isfinite(targets[1, genes[1]]))
    assert int((~torch.isfinite(targets)).sum()) == 1


# --------------------------------------------------------------------------- 6. no extra traffic
def test_fused_scan_allocates_one_block_and_one_buffer(pa, dev):
    """a 16-gene scan at N = 2000: beyond the steady state (cached workspaces, laid-out parameters) the fused scan holds
    the solver's output block, its initial-state buffer and nothing of that size; the eager path (a stacked copy of the
    initial states, |difference| temporaries) goes over the same figure.
    n = 18 inputs per gene: PyTorch's caching allocator may hand out a block of 10 MiB or more as whole 2 MiB units
    and count the unit's unused end (up to 1 MiB, depending on its version and settings) as allocated, which has nothing
    to do with this package; with n = 18 the output block (23 040 000 bytes) ends 28 672 bytes short of its 11 units,
    less than half of the 64 000-byte workspace term that is the budget's slack.  The cache is emptied before each
    measurement so that no larger left-over block is handed out in place of a fresh one."""
    from phoenix_amd import _lib
    N, H, n, k, T = 2000, 40, 18, 8, 10
    genes = list(range(0, 16 * 100, 100))
    net = make_net(pa, dev, rand_params(N, H, seed=21, std=0.6 / np.sqrt(N)))
    kw = dict(n_random_inputs_per_gene=n, device=dev, genes=genes, genes_per_launch=k)
    block = T * 2 * k * n * N * 4
    inits = 2 * k * n * N * 4
    ws = _lib.load().phx_influence_workspace_bytes(T, k, n, N)
    budget = block + inits + ws
    grown = {}
    for fused in (True, False):
        torch.manual_seed(1)
        pa.gene_influence_scores(net, N, "dopri5", fused=fused, **kw)        # steady state: workspaces, parameter layout
        torch.cuda.synchronize()
        torch.cuda.empty_cache()
        torch.cuda.reset_peak_memory_stats()
        base = torch.cuda.memory_allocated()
        torch.manual_seed(1)
        pa.gene_influence_scores(net, N, "dopri5", fused=fused, **kw)
        torch.cuda.synchronize()
        grown[fused] = torch.cuda.max_memory_allocated() - base
    print("peak growth of a 16-gene scan at N=2000: fused %d bytes, eager %d bytes, budget %d (block %d + inits %d + "
          "workspace %d)" % (grown[True], grown[False], budget, block, inits, ws))
    assert grown[True] < budget
    assert grown[False] > budget
