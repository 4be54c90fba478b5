"""Matrix-free products with the inferred network on the MI355X: `effects_apply` (phx_effects_apply through
phoenix_amd.engine) against the matrix that `effects_matrix` / `jacobian_matrix` return, brought to the host, and `apply_ref`
of it (tests/test_apply_cpu.py, pinned there to a brute-force loop); `network_propagation` against `propagation_reference` of
that matrix.  Neither the matrix nor the references are code under test.  The kernel promises the matrix's own bits as
weights, so the only error is that of a float32 dot product: entry by entry
    |out - ref64| <= 1.01 (N + 1) 2^-24 sum |w| |V|
(the worst case for at most N terms in any order, the form of test_neighbors_gpu.strength_ratio), exactly +0 for a line
without eligible entries, and exact equality where every partial sum is a small integer.  Shapes are those of
tests/test_edges_gpu.py, the smallest at which the tiling can go wrong.  Every test prints what it measured before it asserts
(run with -s).
Measured on an MI355X: products, largest |error| / bar 0.018 over candidates, thresholds and 1, 2, 3 segments; propagation,
largest |score - ref| / bar 7.6e-5 (21 steps) and 4.4e-6 (PageRank, 90 steps), |sum - 1| at most 2.2e-7, 3999 ... 6256 gene
pairs ranked as the reference ranks them; a 20-step propagation at N = 2000 grows the device memory by 76 288 bytes."""
import numpy as np
import pytest
import torch

from conftest import load_golden, sub
from test_apply_cpu import apply_lists, apply_ref, lines_of
from test_edges_cpu import select_ref
from test_edges_gpu import MODES, SHAPES, TINY, matrices
from test_effects_gpu import case

pytestmark = pytest.mark.gpu

AXES = ("target", "regulator")
WEIGHTS = ("value", "abs", "unit")
U = 2.0 ** -24


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "these tests need the MI355X"
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def pa():
    import phoenix_amd
    return phoenix_amd


def apply_of(pa, net, yd, mode, v, **kw):
    if mode == "effects":
        return pa.effects_apply(net, v, **kw)
    return pa.effects_apply(net, v, y=yd, reduce=mode, **kw)


def block(N, R, seed, dev, integers=False):
    """(V float32 numpy [N, R], the same on the device): normal draws, or integers in [-8, 8]"""
    rng = np.random.default_rng(seed)
    V = (rng.integers(-8, 9, size=(N, R)) if integers else rng.standard_normal((N, R))).astype(np.float32)
    return V, torch.from_numpy(V).to(dev)


def ratio_of(got, ref, N):
    """the largest |got - out64| / bar over the entries with a positive bar, bar = 1.01 (N + 1) 2^-24 scale; the entries of
    lines without an eligible entry must be +0 to the bit, and where the bar is 0 (every product is 0) the result is 0"""
    out, scale, count = ref
    assert got.dtype == torch.float32 and got.is_cuda
    g = got.cpu().numpy().reshape(out.shape)
    assert np.all(g[count == 0].view(np.uint32) == 0)
    assert np.all(g[scale == 0] == 0)
    live = scale > 0
    if not live.any():
        return 0.0
    return float(np.max(np.abs(g.astype(np.float64) - out)[live] / (1.01 * (N + 1) * U * scale[live])))


# --------------------------------------------------------------------------- 1. against the matrix
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("N,H,B", SHAPES)
def test_products_equal_apply_ref_of_the_matrix(pa, dev, N, H, B, mode):
    net, yd, mats = matrices(pa, dev, N, H, B)
    M = mats[mode]
    V, Vd = block(N, 5, N + H, dev)
    report, worst = [], 0.0
    for of in AXES:
        for orient in (False, True):
            for diagonal in (False, True):
                lists = lines_of(M, of=of, orient=orient, diagonal=diagonal)
                for weight in WEIGHTS:
                    got = apply_of(pa, net, yd, mode, Vd, of=of, weight=weight, orient=orient, diagonal=diagonal)
                    assert tuple(got.shape) == (N, 5)
                    ratio = ratio_of(got, apply_lists(lists, V, weight), N)
                    worst = max(worst, ratio)
                    report.append((of, orient, diagonal, weight, int(lists[2].sum()), round(ratio, 4)))
    print("N=%d H=%d B=%d %s: largest error / bar %.4f; (of, orient, diagonal, weight, eligible, error / bar) %s"
          % (N, H, B, mode, worst, report))
    assert all(r[4] > N // 2 for r in report)
    assert worst <= 1.0, [r for r in report if r[5] > 1.0]


# --------------------------------------------------------------------------- 2. exact cases
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("N,H,B", SHAPES)
def test_unit_weights_on_integers_are_exact(pa, dev, N, H, B, mode):
    """every partial sum of weight="unit" on integers in [-8, 8] is an integer below 8 N < 2^24: exact in float32 in any order"""
    net, yd, mats = matrices(pa, dev, N, H, B)
    M = mats[mode]
    V, Vd = block(N, 5, N + B, dev, integers=True)
    ones = torch.ones(N, dtype=torch.float32, device=dev)
    n = 0
    for of in AXES:
        for orient in (False, True):
            for diagonal in (False, True):
                kw = dict(of=of, orient=orient, diagonal=diagonal)
                gene, _, count = lines_of(M, **kw)
                want = np.zeros((N, 5), np.int64)
                for line in range(N):
                    want[line] = V[gene[line, :count[line]]].astype(np.int64).sum(axis=0)
                got = apply_of(pa, net, yd, mode, Vd, weight="unit", **kw).cpu().numpy()
                assert np.array_equal(got.astype(np.int64), want) and np.array_equal(got, np.rint(got)), (mode, kw)
                # the all-ones vector counts the eligible entries: the degree effects_neighbors reports for the same selection
                deg = apply_of(pa, net, yd, mode, ones, weight="unit", **kw)
                nb = pa.effects_neighbors(net, 1, **kw) if mode == "effects" else \
                    pa.effects_neighbors(net, 1, y=yd, reduce=mode, **kw)
                assert tuple(deg.shape) == (N,) and torch.equal(deg, nb.count.to(torch.float32)), (mode, kw)
                assert np.array_equal(deg.cpu().numpy().astype(np.int64), count)
                n += 1
    print("N=%d H=%d B=%d %s: %d selections exact on integers, degrees equal effects_neighbors(...).count" % (N, H, B, mode, n))


# --------------------------------------------------------------------------- 3. determinism
def bits(x):
    return x.cpu().numpy().view(np.uint32)


@pytest.mark.parametrize("N,H,B", [(97, 7, 5), (130, 40, 2)])
def test_the_bits_of_a_column_do_not_depend_on_its_block(pa, dev, N, H, B):
    net, yd, _ = matrices(pa, dev, N, H, B)
    _, Vd = block(N, 33, 3 * N, dev)
    n = 0
    for mode in ("effects", "mean_abs"):
        for of in AXES:
            for weight, orient in (("value", False), ("abs", True)):
                kw = dict(of=of, weight=weight, orient=orient)
                five = apply_of(pa, net, yd, mode, Vd[:, :5].contiguous(), **kw)
                again = apply_of(pa, net, yd, mode, Vd[:, :5].contiguous(), **kw)
                assert np.array_equal(bits(five), bits(again)), (mode, kw)                       # two calls
                wide = apply_of(pa, net, yd, mode, Vd, **kw)                                     # 33 columns: 32 + 1
                assert tuple(wide.shape) == (N, 33)
                assert np.array_equal(bits(wide[:, :5]), bits(five)), (mode, kw)
                for c in (0, 1, 2, 3, 4, 17, 31, 32):
                    alone = apply_of(pa, net, yd, mode, Vd[:, c].contiguous(), **kw)             # R = 1, as a vector
                    assert tuple(alone.shape) == (N,)
                    assert np.array_equal(bits(alone), bits(wide[:, c])), (mode, kw, c)
                    column = apply_of(pa, net, yd, mode, Vd[:, c:c + 1], **kw)                   # ... and as a [N, 1] view
                    assert np.array_equal(bits(column[:, 0]), bits(alone)), (mode, kw, c)
                n += 1
    print("N=%d: %d selections: two calls, R = 5 against five R = 1, and a 33-column block against its columns agree bit for bit"
          % (N, n))


@pytest.mark.parametrize("N,H,B", [(130, 40, 2), (200, 200, 2)])
def test_the_segments_of_the_streamed_dimension(pa, dev, N, H, B, monkeypatch):
    net, yd, mats = matrices(pa, dev, N, H, B)
    V, Vd = block(N, 5, N + 1, dev)
    Vi, Vid = block(N, 5, N + 2, dev, integers=True)
    worst = 0.0
    for mode in ("effects", "mean_abs"):
        for of in AXES:
            for orient in (False, True):
                kw = dict(of=of, orient=orient)
                lists = lines_of(mats[mode], **kw)
                exact = []
                for s in ("1", "2", "3"):
                    monkeypatch.setenv("PHX_NEIGHBORS_SEGMENTS", s)
                    a = apply_of(pa, net, yd, mode, Vid, weight="unit", **kw)
                    b = apply_of(pa, net, yd, mode, Vid, weight="unit", **kw)
                    assert np.array_equal(bits(a), bits(b)), (mode, kw, s)
                    exact.append(a)
                    for weight in ("value", "abs"):
                        f = apply_of(pa, net, yd, mode, Vd, weight=weight, **kw)
                        assert np.array_equal(bits(f), bits(apply_of(pa, net, yd, mode, Vd, weight=weight, **kw)))
                        worst = max(worst, ratio_of(f, apply_lists(lists, V, weight), N))
                want = apply_lists(lists, Vi, "unit")[0]
                for a in exact:
                    assert np.array_equal(bits(a), bits(exact[0])) and np.array_equal(a.cpu().numpy().astype(np.float64), want)
    print("N=%d H=%d: 1, 2 and 3 segments give identical exact results; largest float error / bar %.4f" % (N, H, worst))
    assert worst <= 1.0


# --------------------------------------------------------------------------- 4. candidates and threshold
@pytest.mark.parametrize("mode", ["effects", "mean_abs"])
def test_candidates_and_threshold(pa, dev, mode):
    N, H, B = 130, 40, 2
    net, yd, mats = matrices(pa, dev, N, H, B)
    M = mats[mode]
    V, Vd = block(N, 5, 77, dev)
    first = list(range(0, 64, 3))                                                    # candidates in the first 64 genes only:
    regulators = list(range(0, N, 3))                                                # the other line tiles hold none
    targets = [j for j in range(N) if not 64 <= j < 128 and j % 5 != 1]            # a whole tile without a candidate
    mags = np.sort(np.abs(select_ref(M, threshold=TINY)[2]))
    tau = float(mags[len(mags) // 2])                                                # a magnitude that occurs: inclusive
    between = (tau + float(np.nextafter(np.float32(tau), np.float32(np.inf)))) / 2   # strictly between two float32 values
    report = []
    for of in AXES:
        for orient in (False, True):
            for sel in (dict(regulators=regulators), dict(targets=targets), dict(regulators=regulators, targets=targets),
                        dict(regulators=first), dict(targets=first), dict(regulators=first, targets=first),
                        dict(regulators=torch.tensor(regulators + regulators[:5], device=dev), targets=np.array(targets)),
                        dict(threshold=tau), dict(threshold=between), dict(regulators=regulators, targets=targets, threshold=tau),
                        dict(regulators=[7], targets=[7, 70]), dict(regulators=[], targets=targets)):
                plain = {n: (v.cpu().tolist() if isinstance(v, torch.Tensor) else v) for n, v in sel.items()}
                lists = lines_of(M, of=of, orient=orient, **plain)
                for weight in ("abs", "unit"):
                    got = apply_of(pa, net, yd, mode, Vd, of=of, weight=weight, orient=orient, **sel)
                    ratio = ratio_of(got, apply_lists(lists, V, weight), N)
                    report.append((of, orient, sorted(sel), weight, int(lists[2].sum()), round(ratio, 4)))
                    outside = [n for n in range(N) if n not in plain.get("targets" if of == "target" else "regulators", range(N))]
                    assert np.all(got.cpu().numpy()[outside].view(np.uint32) == 0)
    print("%s: (of, orient, selection, weight, eligible, error / bar) %s" % (mode, report))
    assert all(r[5] <= 1.0 for r in report), [r for r in report if r[5] > 1.0]
    # the threshold is inclusive, and the next float32 above it excludes the entries at it: the unit weights count them
    ones = torch.ones(N, dtype=torch.float32, device=dev)
    at = int(apply_of(pa, net, yd, mode, ones, weight="unit", threshold=tau).sum())
    above = int(apply_of(pa, net, yd, mode, ones, weight="unit", threshold=between).sum())
    assert at == int((mags >= np.float32(tau)).sum()) and above == int((mags > np.float32(tau)).sum()) and at > above > 0
    got = apply_of(pa, net, yd, mode, Vd, threshold=3e38)
    assert np.all(bits(got) == 0)


# --------------------------------------------------------------------------- 5. non-finite values
def test_non_finite_entries_and_non_finite_vectors(pa, dev):
    N, H, B = 37, 5, 3
    net, yd, mats = matrices(pa, dev, N, H, B)
    zero = np.nonzero(np.all(mats["effects"] == 0, axis=0))[0]
    assert len(zero) >= 2
    V, Vd = block(N, 3, 5, dev)
    for mode in MODES:                                       # nothing regulates the genes of the zero columns
        got = apply_of(pa, net, yd, mode, Vd, of="target", weight="abs")
        assert np.all(bits(got)[zero] == 0)
    # a NaN in one regulator's column of Ws (a gene whose own column is live): its whole row of the matrix is NaN
    r = int(min(set(range(N)) - set(zero.tolist())))
    p = {n: v.copy() for n, v in sub(load_golden("g21_edges"), "p_").items()}
    p["Ws"][2, r] = np.nan
    _, net2, _, _, yd2, _ = case(pa, dev, N, H, B, p=p)
    q = int(max(set(range(N)) - set(zero.tolist()) - {r}))   # a live gene whose entry of V is not finite
    Vn = V.copy()
    Vn[q, 0], Vn[q, 1] = np.nan, np.inf
    Vnd = torch.from_numpy(Vn).to(dev)
    others = [g for g in range(N) if g != q]
    seen = 0
    for mode in MODES:
        M = (pa.effects_matrix(net2) if mode == "effects" else pa.jacobian_matrix(net2, yd2, reduce=mode)).cpu().numpy()
        live = [j for j in range(N) if j not in zero]
        assert np.all(np.isnan(M[r, live]))
        for of in AXES:
            for orient in (False, True):
                for weight in WEIGHTS:
                    kw = dict(of=of, weight=weight, orient=orient)
                    # a NaN or Inf entry of M never reaches out
                    got = apply_of(pa, net2, yd2, mode, Vd, **kw)
                    assert bool(torch.isfinite(got).all()), (mode, kw)
                    assert ratio_of(got, apply_ref(M, V, **kw), N) <= 1.0, (mode, kw)
                    # a NaN of V[q] appears in exactly the lines with an eligible entry at q; so does the Inf, as Inf or NaN
                    got = apply_of(pa, net2, yd2, mode, Vnd, **kw).cpu().numpy()
                    ref = apply_ref(M, Vn, **kw)[0]
                    assert np.array_equal(np.isnan(got[:, 0]), np.isnan(ref[:, 0])), (mode, kw)
                    assert np.array_equal(np.isfinite(got[:, 1]), np.isfinite(ref[:, 1])), (mode, kw)
                    assert np.all(np.isfinite(got[:, 2]))
                    seen += int(np.isnan(ref[:, 0]).sum())
                    # with q taken out of the streamed side's candidates it appears nowhere
                    out = dict(regulators=others) if of == "target" else dict(targets=others)
                    got = apply_of(pa, net2, yd2, mode, Vnd, **kw, **out)
                    assert bool(torch.isfinite(got).all()), (mode, kw)
    print("a NaN of V reached %d lines over all selections, the reference's pattern each time; NaN entries of M none" % seen)
    assert seen > 0


# --------------------------------------------------------------------------- 6. propagation
PROP_FACTOR = 3     # see propagation_bar


def propagation_bar(N, steps):
    """The bar on |score - ref| per entry.  The walk's map contracts the 1-norm by (1 - restart) < 1, so the distance of the
    float32 walk from the float64 one after any number of steps is at most the sum of the steps' own rounding errors in the
    1-norm.  One step's error has three parts, each at most the bar of test 1 summed over the lines, 1.01 (N + 1) 2^-24
    times sum |w| |x| = the walk's mass = 1: the product itself; the strengths that scale it (the same kernel on the ones
    vector: a relative error of that size in every 1 / s); and everything element-wise around them (the seeds' rounding, the
    quotient, the two scalings, the sum of the dangling mass over at most N genes: at most N + 8 roundings).  Factor 3,
    times the step count."""
    return PROP_FACTOR * steps * 1.01 * (N + 1) * U


@pytest.mark.parametrize("N,H,B", [(97, 7, 5), (130, 40, 2)])
def test_propagation_equals_the_reference_walk_on_the_matrix(pa, dev, N, H, B):
    net, yd, mats = matrices(pa, dev, N, H, B)
    rng = np.random.default_rng(N)
    two = rng.random((N, 2)).astype(np.float32)
    two[rng.random((N, 2)) < 0.7] = 0.0
    two[3, 0], two[5, 1] = 1.0, 2.0
    genes = [2, 11, N - 1]
    worst, report = 0.0, []
    for mode in ("effects", "mean_abs"):
        M = mats[mode]
        sel = dict(threshold=float(np.quantile(np.abs(M[M != 0]), 0.8)))      # a sparse network: hubs and dangling genes
        for direction in ("downstream", "upstream"):
            for weight in ("abs", "unit"):
                for orient in (False, True):
                    for seeds in (genes, torch.from_numpy(two).to(dev)):
                        kw = dict(restart=0.5, direction=direction, weight=weight, orient=orient, **sel)
                        got = pa.network_propagation(net, seeds, **kw) if mode == "effects" else \
                            pa.network_propagation(net, seeds, y=yd, reduce=mode, **kw)
                        ref = pa.propagation_reference(M, seeds, **kw)
                        R = 1 if seeds is genes else 2
                        assert got.iterations == ref.iterations == 21
                        assert got.score.is_cuda and got.score.dtype == torch.float32
                        assert tuple(got.score.shape) == ((N,) if R == 1 else (N, 2)) == ref.score.shape
                        s = got.score.cpu().numpy().astype(np.float64).reshape(N, R)
                        sums = np.abs(s.sum(axis=0) - 1.0).max()
                        ratio = float(np.abs(s - ref.score.reshape(N, R)).max() / propagation_bar(N, got.iterations))
                        worst = max(worst, ratio)
                        residual = np.max(got.residual)
                        report.append((mode, direction, weight, orient, R, "%.2e" % sums, "%.2e" % ratio, "%.2e" % residual))
                        assert sums <= got.iterations * N * U, report[-1]
                        assert residual <= 1e-6 and np.max(ref.residual) <= 1e-6, report[-1]
                        assert np.all(s >= 0)
    print("N=%d: largest |score - ref| / bar %.3e (bar = %d x steps x 1.01 (N + 1) 2^-24); (mode, direction, weight, orient, "
          "columns, |sum - 1|, error / bar, residual) %s" % (N, worst, PROP_FACTOR, report))
    assert worst <= 1.0


@pytest.mark.parametrize("N,H,B", [(97, 7, 5), (130, 40, 2)])
def test_pagerank_ranks_the_genes_as_the_reference_does(pa, dev, N, H, B):
    net, yd, mats = matrices(pa, dev, N, H, B)
    for mode in ("effects", "mean_abs"):
        got = pa.network_propagation(net, restart=0.15) if mode == "effects" else \
            pa.network_propagation(net, restart=0.15, y=yd, reduce=mode)
        ref = pa.propagation_reference(mats[mode], restart=0.15)
        assert got.iterations == ref.iterations == 90 and tuple(got.score.shape) == (N,) and np.ndim(got.residual) == 0
        bar = propagation_bar(N, got.iterations)
        s = got.score.cpu().numpy().astype(np.float64)
        ratio = float(np.abs(s - ref.score).max() / bar)
        apart = ref.score[:, None] - ref.score[None, :] > bar           # pairs (a, b) the reference ranks a above b, clearly
        same = (s[:, None] > s[None, :])[apart]
        print("N=%d %s: PageRank |score - ref| / bar %.3e; %d gene pairs lie further apart than the bar, %d ranked alike; "
              "|sum - 1| %.2e, residual %.2e" % (N, mode, ratio, int(apart.sum()), int(same.sum()), abs(s.sum() - 1), got.residual))
        assert ratio <= 1.0 and got.residual <= 1e-6 and abs(s.sum() - 1) <= got.iterations * N * U
        assert apart.sum() > 0 and same.all()


# --------------------------------------------------------------------------- 7. beyond the steady state
def test_a_propagation_allocates_no_matrix(pa, dev):
    N, H = 2000, 40
    _, net, _, _, yd, _ = case(pa, dev, N, H, 2)
    chunk = 2048 * N * 4                                    # one 2048-row chunk of the matrix the composition would form
    for kw in (dict(), dict(y=yd, orient=True)):
        first = pa.network_propagation(net, [1, 2, 3], iterations=20, **kw)    # steady state: parameter layout, workspace
        torch.cuda.synchronize()
        assert first.iterations == 20
        del first
        torch.cuda.empty_cache()
        torch.cuda.reset_peak_memory_stats()
        base = torch.cuda.memory_allocated()
        res = pa.network_propagation(net, [1, 2, 3], iterations=20, **kw)
        torch.cuda.synchronize()
        grown = torch.cuda.max_memory_allocated() - base
        assert abs(float(res.score.sum()) - 1.0) <= 20 * N * U
        del res
        print("peak growth of a 20-step propagation (%s) at N=%d: %d bytes (one 2048-row chunk of the matrix: %d)"
              % (sorted(kw), N, grown, chunk))
        assert grown < chunk
