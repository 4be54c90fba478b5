"""Per-gene neighbour lists on the MI355X: `effects_neighbors` (phx_effects_neighbors through phoenix_amd.engine) against the
matrix that `effects_matrix` / `jacobian_matrix` return, brought to the host, and `neighbors_ref` of it
(tests/test_neighbors_cpu.py, pinned there to a brute-force loop and to the reference's get_link_list).  Neither is code under
test, and the kernel promises the matrix's own bits, so lists, values and counts are compared exactly; the strength is a
float32 sum and is held to the worst-case bound of such a sum.  Shapes are those of tests/test_edges_gpu.py, the smallest at
which the tiling can go wrong: (33, 1, 1) one ragged tile, k = 64 exceeds every line; (37, 5, 3) the golden G21 with its zero
columns; (97, 7, 5) 2 x 2 ragged tiles; (130, 40, 2) three tiles, lists merge across full and ragged tiles and across three
segments; (200, 200, 2) more than 32 hidden rows.  Every test prints what it measured before it asserts (run with -s)."""
import numpy as np
import pytest
import torch

from conftest import load_golden
from test_edges_cpu import select_ref
from test_edges_gpu import MODES, SHAPES, TINY, matrices
from test_effects_gpu import case
from test_gpu_parity import rand_params
from test_neighbors_cpu import golden_cases, grouped, neighbors_ref

pytestmark = pytest.mark.gpu

KS = (1, 5, 64)
AXES = ("target", "regulator")


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "these tests need the MI355X"
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def pa():
    import phoenix_amd
    return phoenix_amd


def neighbors_of(pa, net, yd, mode, k, **kw):
    if mode == "effects":
        return pa.effects_neighbors(net, k, **kw)
    return pa.effects_neighbors(net, k, y=yd, reduce=mode, **kw)


def lists_equal(got, ref):
    """gene, the bits of value (padding -1 / +0 included) and count"""
    N, k = ref[0].shape
    assert got.gene.dtype == got.count.dtype == torch.int64 and got.value.dtype == got.strength.dtype == torch.float32
    assert all(x.is_cuda for x in got)
    assert tuple(got.gene.shape) == tuple(got.value.shape) == (N, k) and tuple(got.count.shape) == tuple(got.strength.shape) == (N,)
    return (np.array_equal(got.gene.cpu().numpy(), ref[0]) and
            np.array_equal(got.value.cpu().numpy().view(np.uint32), ref[1].view(np.uint32)) and
            np.array_equal(got.count.cpu().numpy(), ref[2]))


def strength_ratio(got, ref, N):
    """the largest |strength - s64| / bar, bar = 1.01 N 2^-24 s64: the worst-case error of a float32 sum of at most N
    non-negative terms in any order (gamma_{n-1}, n <= 65535); lines without entries must be exactly 0"""
    s = got.strength.cpu().numpy().astype(np.float64)
    s64 = ref[3]
    assert np.all(s[s64 == 0] == 0)
    live = s64 > 0
    if not live.any():
        return 0.0
    return float(np.max(np.abs(s - s64)[live] / (1.01 * N * 2.0 ** -24 * s64[live])))


# --------------------------------------------------------------------------- 1, 2. lists, values, counts and strengths
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("N,H,B", SHAPES)
def test_lists_counts_and_strengths_equal_neighbors_ref_of_the_matrix(pa, dev, N, H, B, mode):
    net, yd, mats = matrices(pa, dev, N, H, B)
    M = mats[mode]
    report, worst = [], 0.0
    for of in AXES:
        for orient in (False, True):
            for diagonal in (False, True):
                for k in KS:
                    kw = dict(of=of, orient=orient, diagonal=diagonal)
                    got = neighbors_of(pa, net, yd, mode, k, **kw)
                    ref = neighbors_ref(M, k, **kw)
                    ratio = strength_ratio(got, ref, N)
                    worst = max(worst, ratio)
                    report.append((of, orient, diagonal, k, int(ref[2].sum()), lists_equal(got, ref), ratio <= 1.0))
    print("N=%d H=%d B=%d %s: largest strength error / bar %.4f; (of, orient, diagonal, k, eligible, lists identical, strength "
          "inside) %s" % (N, H, B, mode, worst, report))
    assert all(r[4] > N // 2 for r in report)
    assert all(r[5] for r in report), [r for r in report if not r[5]]
    assert all(r[6] for r in report), [r for r in report if not r[6]]


# --------------------------------------------------------------------------- 3. candidates and threshold
@pytest.mark.parametrize("mode", ["effects", "mean_abs"])
def test_candidates_and_threshold(pa, dev, mode):
    N, H, B = 130, 40, 2
    net, yd, mats = matrices(pa, dev, N, H, B)
    M = mats[mode]
    regulators = list(range(0, N, 3))
    targets = [j for j in range(N) if not 64 <= j < 128 and j % 5 != 1]            # a whole tile without a candidate
    mags = np.sort(np.abs(select_ref(M, threshold=TINY)[2]))
    tau = float(mags[len(mags) // 2])                                                # a magnitude that occurs: inclusive
    between = (tau + float(np.nextafter(np.float32(tau), np.float32(np.inf)))) / 2   # strictly between two float32 values
    report = []
    for of in AXES:
        for orient in (False, True):
            for sel in (dict(regulators=regulators), dict(targets=targets), dict(regulators=regulators, targets=targets),
                        dict(regulators=torch.tensor(regulators + regulators[:5], device=dev), targets=np.array(targets)),
                        dict(threshold=tau), dict(threshold=between), dict(regulators=regulators, targets=targets, threshold=tau),
                        dict(regulators=[7], targets=[7, 70]), dict(regulators=[], targets=targets)):
                for k in (5, 64):
                    got = neighbors_of(pa, net, yd, mode, k, of=of, orient=orient, **sel)
                    plain = {n: (v.cpu().tolist() if isinstance(v, torch.Tensor) else v) for n, v in sel.items()}
                    ref = neighbors_ref(M, k, of=of, orient=orient, **plain)
                    ratio = strength_ratio(got, ref, N)
                    report.append((of, orient, sorted(sel), k, int(ref[2].sum()), lists_equal(got, ref), ratio <= 1.0))
                    outside = [n for n in range(N) if n not in plain.get("targets" if of == "target" else "regulators", range(N))]
                    assert np.all(got.count.cpu().numpy()[outside] == 0) and np.all(got.gene.cpu().numpy()[outside] == -1)
                    assert np.all(got.value.cpu().numpy()[outside].view(np.uint32) == 0)
    print("%s: (of, orient, selection, k, eligible, lists identical, strength inside) %s" % (mode, report))
    assert all(r[5] and r[6] for r in report), [r for r in report if not (r[5] and r[6])]
    # the threshold is inclusive, and the next float32 above it excludes the entries at it
    at = neighbors_ref(M, 5, threshold=tau)[2].sum(), neighbors_ref(M, 5, threshold=between)[2].sum()
    assert at[0] > at[1] > 0
    got = neighbors_of(pa, net, yd, mode, 5, threshold=3e38)
    assert int(got.count.sum()) == 0 and bool((got.gene == -1).all())


# --------------------------------------------------------------------------- 4. ties
@pytest.mark.parametrize("mode", ["effects", "mean_abs"])
def test_a_tie_at_the_cut_goes_to_the_lower_index(pa, dev, mode):
    """genes 70 and 129 copy gene 3's columns of Ws and Wp and its state: rows 3, 70 and 129 of the matrix are bitwise equal,
    so every target's column holds a three-way tie across tiles (and segments); genes 80 and 128 copy gene 5's column of
    WaT and its multiplier: columns 5, 80 and 128 are equal, a tie within and across tiles for every regulator's row"""
    N, H, B = 130, 40, 2
    p = rand_params(N, H, seed=N + H, std=0.6 / np.sqrt(N))
    p["g"][[3, 5]] = 0.9, 0.8
    for c in (70, 129):
        p["Ws"][:, c], p["Wp"][:, c] = p["Ws"][:, 3], p["Wp"][:, 3]
    for c in (80, 128):
        p["Wa"][c, :], p["g"][c] = p["Wa"][5, :], p["g"][5]
    _, net, _, _, yd, _ = case(pa, dev, N, H, B, p=p)
    for c in (70, 129):
        yd[:, c] = yd[:, 3]
    M = (pa.effects_matrix(net) if mode == "effects" else pa.jacobian_matrix(net, yd, reduce=mode)).cpu().numpy()
    off = [j for j in range(N) if j not in (3, 70, 129)]
    assert np.array_equal(M[3, off].view(np.uint32), M[70, off].view(np.uint32))
    assert np.array_equal(M[3, off].view(np.uint32), M[129, off].view(np.uint32))
    off = [i for i in range(N) if i not in (5, 80, 128)]
    assert np.array_equal(M[off, 5].view(np.uint32), M[off, 80].view(np.uint32))
    assert np.array_equal(M[off, 5].view(np.uint32), M[off, 128].view(np.uint32))
    seen = 0
    for of, trio in (("target", (3, 70, 129)), ("regulator", (5, 80, 128))):
        full = neighbors_ref(M, 64, of=of)[0]
        # where the trio stands in every line that ranks all three among its 64 strongest; the cuts that fall inside one
        first = {}
        for n in range(N):
            where = [int(np.nonzero(full[n] == t)[0][0]) for t in trio if t in full[n]]
            if len(where) == 3:
                assert where == [where[0], where[0] + 1, where[0] + 2], (of, n, where)      # equal magnitudes, index order
                first[n] = where[0]
        ks = sorted({w + d for w in first.values() for d in (1, 2) if w + d <= 64})[:10]
        assert len(ks) >= 4
        for k in ks:
            got = neighbors_of(pa, net, yd, mode, k, of=of)
            ref = neighbors_ref(M, k, of=of)
            assert lists_equal(got, ref), (of, k)
            g = got.gene.cpu().numpy()
            for n, w in first.items():
                if w < k <= w + 2:                    # the cut falls between the copies: the smaller indices are kept
                    assert [t for t in trio if t in g[n]] == list(trio[:k - w]), (of, k, n)
                    seen += 1
    print("%s: %d (line, k) pairs cut a bitwise three-way tie; the lower indices were kept" % (mode, seen))
    assert seen >= 8


# --------------------------------------------------------------------------- 5. zero columns and non-finite entries
def test_zero_columns_and_non_finite_entries(pa, dev):
    N, H, B = 37, 5, 3
    net, yd, mats = matrices(pa, dev, N, H, B)
    zero = np.nonzero(np.all(mats["effects"] == 0, axis=0))[0]
    assert len(zero) >= 2
    for mode in MODES:
        got = neighbors_of(pa, net, yd, mode, 64, of="target")
        assert np.all(got.count.cpu().numpy()[zero] == 0) and np.all(got.strength.cpu().numpy()[zero] == 0)
        assert np.all(got.gene.cpu().numpy()[zero] == -1)
        got = neighbors_of(pa, net, yd, mode, 64, of="regulator")
        assert not np.isin(got.gene.cpu().numpy(), zero).any()
    # a NaN in one regulator's column of Ws (a gene whose own column is live): its whole row of the matrix is NaN
    r = int(min(set(range(N)) - set(zero.tolist())))
    from conftest import sub
    p = {n: v.copy() for n, v in sub(load_golden("g21_edges"), "p_").items()}
    p["Ws"][2, r] = np.nan
    _, net2, _, _, yd2, _ = case(pa, dev, N, H, B, p=p)
    for mode in MODES:
        M = (pa.effects_matrix(net2) if mode == "effects" else pa.jacobian_matrix(net2, yd2, reduce=mode)).cpu().numpy()
        live = [j for j in range(N) if j not in zero]
        assert np.all(np.isnan(M[r, live]))
        for of in AXES:
            for orient in (False, True):
                got = neighbors_of(pa, net2, yd2, mode, 64, of=of, orient=orient)
                ref = neighbors_ref(M, 64, of=of, orient=orient)
                assert lists_equal(got, ref) and strength_ratio(got, ref, N) <= 1.0, (mode, of, orient)
                assert not (got.gene.cpu().numpy() == r).any() if of == "target" else int(got.count[r]) == 0
                assert bool(torch.isfinite(got.value).all()) and bool(torch.isfinite(got.strength).all())
        # under orient the NaN costs its partners the comparison: nothing points at that gene either
        got = neighbors_of(pa, net2, yd2, mode, 64, of="target", orient=True)
        plain = neighbors_of(pa, net2, yd2, mode, 64, of="target")
        print("%s: regulators of gene %d, whose row is NaN: %d plain, %d under orient" % (mode, r, int(plain.count[r]), int(got.count[r])))
        assert int(plain.count[r]) > 0 and int(got.count[r]) == 0


# --------------------------------------------------------------------------- 6. segments
@pytest.mark.parametrize("N,H,B", [(130, 40, 2), (200, 200, 2)])
def test_the_segments_of_the_streamed_dimension_do_not_change_the_lists(pa, dev, N, H, B, monkeypatch):
    net, yd, mats = matrices(pa, dev, N, H, B)
    worst = 0.0
    for mode in ("effects", "mean_abs"):
        for of in AXES:
            for orient in (False, True):
                ref = neighbors_ref(mats[mode], 5, of=of, orient=orient)
                runs = []
                for s in ("1", "2", "3"):
                    monkeypatch.setenv("PHX_NEIGHBORS_SEGMENTS", s)
                    a = neighbors_of(pa, net, yd, mode, 5, of=of, orient=orient)
                    b = neighbors_of(pa, net, yd, mode, 5, of=of, orient=orient)
                    assert all(torch.equal(x, z) for x, z in zip(a, b)), (mode, of, orient, s)     # strength included
                    assert lists_equal(a, ref), (mode, of, orient, s)
                    worst = max(worst, strength_ratio(a, ref, N))
                    runs.append(a)
                for a in runs[1:]:
                    assert all(torch.equal(x, z) for x, z in zip(a[:3], runs[0][:3]))
    print("N=%d H=%d: 1, 2 and 3 segments give identical lists and counts; largest strength error / bar %.4f" % (N, H, worst))
    assert worst <= 1.0


# --------------------------------------------------------------------------- 7. against the sibling kernel
@pytest.mark.parametrize("N,H,B", [(33, 1, 1), (37, 5, 3)])
def test_lists_equal_the_grouped_edges_of_effects_edges(pa, dev, N, H, B):
    net, yd, _ = matrices(pa, dev, N, H, B)
    n = 0
    for mode in MODES:
        for orient in (False, True):
            for diagonal in (False, True):
                kw = dict(orient=orient, diagonal=diagonal)
                e = pa.effects_edges(net, threshold=TINY, **kw) if mode == "effects" else \
                    pa.effects_edges(net, threshold=TINY, y=yd, reduce=mode, **kw)
                reg, tgt, val = (x.cpu().numpy() for x in e)        # magnitude descending, then regulator, then target
                for of in AXES:
                    got = neighbors_of(pa, net, yd, mode, 64, of=of, **kw)
                    assert lists_equal(got, grouped(reg, tgt, val, N, 64, of)), (mode, of, kw)
                    n += 1
    print("N=%d: %d neighbour lists equal the grouped output of effects_edges" % (N, n))


# --------------------------------------------------------------------------- 8. the reference's own ranking
def test_golden_ranking(pa, dev):
    net, _, mats = matrices(pa, dev, 37, 5, 3)
    M = mats["effects"]
    n = 0
    for tag, ctag, _, cand, (reg, tgt, score) in golden_cases():
        for of in AXES:
            got = pa.effects_neighbors(net, 5, of=of, regulators=cand, orient=tag == "masked")
            gene, mag, count = grouped(reg, tgt, score, 37, 5, of)
            g = got.gene.cpu().numpy()
            print("G23 %s %s of=%s: %d links of the reference, %d counted" % (tag, ctag, of, len(score), int(got.count.sum())))
            assert np.array_equal(g, gene) and np.array_equal(got.count.cpu().numpy(), count)
            # the values are the kernel's own entries, within the rounding bound of the reference's (asserted on the matrix
            # in tests/test_effects_gpu.py); here: they are the matrix's bits at the reference's positions
            line = np.broadcast_to(np.arange(37)[:, None], g.shape)
            i, j = (g, line) if of == "target" else (line, g)
            assert np.array_equal(got.value.cpu().numpy()[g >= 0].view(np.uint32), M[i[g >= 0], j[g >= 0]].view(np.uint32))
            n += 1
    assert n == 8
