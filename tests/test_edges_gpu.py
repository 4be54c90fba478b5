"""Edge extraction on the MI355X: `effects_edges` (phx_effects_edges through phoenix_amd.engine) against the matrix that
`effects_matrix` / `jacobian_matrix` return, brought to the host and selected by `select_ref` (tests/test_edges_cpu.py, pinned
there to the reference's make_mask).  Neither is code under test, and the kernel promises the matrix's own bits, so every
comparison is exact: the same indices in the same order and the same value bits.  Shapes are the smallest at which the tiling
can go wrong: (33, 1, 1) one ragged tile; (37, 5, 3) the golden G21 with its zero columns; (97, 7, 5) 2 x 2 ragged tiles, the
first off-diagonal pair; (130, 40, 2) three tiles, full-full and full-ragged pairs; (200, 200, 2) more than 32 hidden rows.
Every test prints what it measured before it asserts (run with -s to see it)."""
import numpy as np
import pytest
import torch

from conftest import load_golden, sub
from test_edges_cpu import select_ref
from test_effects_cpu import closed_form, kernel_bound
from test_effects_gpu import case
from test_gpu_parity import make_net, rand_params

pytestmark = pytest.mark.gpu

SHAPES = [(33, 1, 1), (37, 5, 3), (97, 7, 5), (130, 40, 2), (200, 200, 2)]
MODES = ("effects", "mean", "mean_abs")
TINY = 1e-45          # rounds up to the smallest positive float32: every eligible entry


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "these tests need the MI355X"
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def pa():
    import phoenix_amd
    return phoenix_amd


_CASES = {}


def matrices(pa, dev, N, H, B):
    """(net, states on the device, {mode: the parent's matrix on the host}) of a shape, computed once and never changed"""
    key = (N, H, B)
    if key not in _CASES:
        p = sub(load_golden("g21_edges"), "p_") if (N, H) == (37, 5) else None
        _, net, _, _, yd, _ = case(pa, dev, N, H, B, p=p)
        M = {"effects": pa.effects_matrix(net).cpu().numpy()}
        for mode in ("mean", "mean_abs"):
            M[mode] = pa.jacobian_matrix(net, yd, reduce=mode).cpu().numpy()
        for m in M.values():
            m.setflags(write=False)
        _CASES[key] = (net, yd, M)
    return _CASES[key]


def edges_of(pa, net, yd, mode, **kw):
    if mode == "effects":
        return pa.effects_edges(net, **kw)
    return pa.effects_edges(net, y=yd, reduce=mode, **kw)


def same(got, ref):
    """indices, order and value bits"""
    i, j, v = ref
    assert got.regulator.dtype == got.target.dtype == torch.int64 and got.value.dtype == torch.float32
    assert got.regulator.is_cuda and got.target.is_cuda and got.value.is_cuda
    return (np.array_equal(got.regulator.cpu().numpy(), i) and np.array_equal(got.target.cpu().numpy(), j) and
            np.array_equal(got.value.cpu().numpy().view(np.uint32), v.view(np.uint32)))


# --------------------------------------------------------------------------- 1. every mode, flag and selection
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("N,H,B", SHAPES)
def test_selection_equals_select_ref_of_the_matrix(pa, dev, N, H, B, mode):
    net, yd, mats = matrices(pa, dev, N, H, B)
    M = mats[mode]
    for orient in (False, True):
        for diagonal in (False, True):
            kw = dict(orient=orient, diagonal=diagonal)
            everything = select_ref(M, threshold=TINY, **kw)
            E = len(everything[2])
            assert E > N // 2
            mags = np.abs(everything[2])
            # a threshold that is one of the magnitudes (inclusive), and one strictly between two float32 neighbours
            k = E // 3
            tau = float(mags[k])
            count = int((mags >= mags[k]).sum())
            between = (float(mags[k]) + float(np.nextafter(mags[k], np.float32(np.inf)))) / 2
            report = []
            for name, sel in (("all", dict(threshold=TINY)), ("threshold", dict(threshold=tau)),
                              ("between", dict(threshold=between)), ("top=1", dict(top=1)), ("top=7", dict(top=7)),
                              ("top>E", dict(top=N * N + 5))):
                got = edges_of(pa, net, yd, mode, **sel, **kw)
                ref = select_ref(M, **sel, **kw)
                report.append((name, len(got.value), len(ref[2]), same(got, ref)))
            print("N=%d H=%d B=%d %s orient=%d diagonal=%d: %d eligible; (selection, got, expected, identical) %s"
                  % (N, H, B, mode, orient, diagonal, E, report))
            assert all(r[3] for r in report), report
            assert report[1][1] == count and report[2][1] == int((mags > mags[k]).sum()) and report[5][1] == E
            # the one-pass form: a list that is exactly large enough, and one that is one entry short
            got = edges_of(pa, net, yd, mode, threshold=tau, max_edges=count, **kw)
            assert same(got, select_ref(M, threshold=tau, **kw))
            if count > 1:
                with pytest.raises(RuntimeError, match=r"\b%d edges qualify" % count):
                    edges_of(pa, net, yd, mode, threshold=tau, max_edges=count - 1, **kw)


def test_two_runs_give_identical_tensors(pa, dev):
    net, yd, _ = matrices(pa, dev, 130, 40, 2)
    for mode in MODES:
        for sel in (dict(top=500), dict(threshold=0.01)):
            a = edges_of(pa, net, yd, mode, orient=True, **sel)
            b = edges_of(pa, net, yd, mode, orient=True, **sel)
            assert len(a.value) > 100
            assert all(torch.equal(x, z) for x, z in zip(a, b)), (mode, sel)


# --------------------------------------------------------------------------- 2. the reference's own network
def test_golden_orientation(pa, dev):
    g = load_golden("g21_edges")
    p, masked = sub(g, "p_"), g["masked"]
    H, N = p["Ws"].shape
    net, _, _ = matrices(pa, dev, N, H, 3)
    got = pa.effects_edges(net, threshold=TINY, orient=True)
    i, j, v = (x.cpu().numpy() for x in got)
    support = np.zeros((N, N), bool)
    support[i, j] = True
    _, A = closed_form(p, "effects")
    err, bound = np.abs(v.astype(np.float64) - masked[i, j]), kernel_bound(H, 0, A)[i, j]
    print("G21: %d edges, the reference keeps %d; worst |value - reference| / bound = %.4f"
          % (len(v), int((masked != 0).sum()), float(np.max(err / bound))))
    assert len(v) == len(set(zip(i.tolist(), j.tolist())))
    assert np.array_equal(support, masked != 0)
    assert np.all(err <= bound)


# --------------------------------------------------------------------------- 3. ties
def test_a_symmetric_model_has_no_orientation(pa, dev):
    """Wp = 0, WaT[:H] = Ws and equal multipliers: effects[i, j] and effects[j, i] are the same chain of the same products,
    so the matrix is symmetric bit for bit and `orient` finds no stronger direction anywhere"""
    N, H = 97, 7
    p = rand_params(N, H, seed=11, std=0.6 / np.sqrt(N))
    p["Wp"][:] = 0
    p["Wa"][:, :H] = p["Ws"].T
    p["g"][:] = 0.75
    net = make_net(pa, dev, p)
    M = pa.effects_matrix(net).cpu().numpy()
    assert np.array_equal(M.view(np.uint32), M.T.copy().view(np.uint32))
    mags = np.sort(np.abs(M[np.triu_indices(N, 1)]))[::-1]
    tau = float(mags[len(mags) // 4])
    pairs = int((mags >= mags[len(mags) // 4]).sum())
    for sel in (dict(threshold=TINY), dict(threshold=tau), dict(top=50)):
        assert len(pa.effects_edges(net, orient=True, **sel).value) == 0
    got = pa.effects_edges(net, threshold=tau)
    print("symmetric model: %d unordered pairs at or above the threshold, %d edges without orient, 0 with" % (pairs, len(got.value)))
    assert len(got.value) == 2 * pairs and same(got, select_ref(M, threshold=tau))
    # every magnitude occurs twice: a cut bin capped at one entry cannot be resolved, and the error says so
    from phoenix_amd import engine
    from phoenix_amd.odenet import params_of
    with pytest.raises(RuntimeError, match="share the magnitude"):
        engine.effects_edges(engine.params_cached(*params_of(net)), "effects", top=51, refine_above=1)


@pytest.mark.parametrize("mode", ["effects", "mean_abs"])
def test_a_tie_at_the_cut_goes_to_the_lower_index(pa, dev, mode):
    """regulators a and b with the same columns of Ws and Wp (and the same states) have identical rows"""
    N, H, B, a, b = 97, 7, 3, 21, 70
    p = rand_params(N, H, seed=13, std=0.6 / np.sqrt(N))
    p["Ws"][:, b], p["Wp"][:, b] = p["Ws"][:, a], p["Wp"][:, a]
    _, net, _, _, yd, _ = case(pa, dev, N, H, B, p=p)
    yd[:, b] = yd[:, a]
    M = (pa.effects_matrix(net) if mode == "effects" else pa.jacobian_matrix(net, yd, reduce=mode)).cpu().numpy()
    i, j, v = select_ref(M, threshold=TINY)
    at = [k for k in range(len(v) - 1) if (i[k], i[k + 1]) == (a, b) and j[k] == j[k + 1] and abs(v[k]) == abs(v[k + 1])]
    assert len(at) > N // 2
    k = at[len(at) // 2]
    got = edges_of(pa, net, yd, mode, top=k + 1)
    print("%s: cut after position %d, between (%d, %d) and (%d, %d) of magnitude %.6e: last edge returned (%d, %d)"
          % (mode, k, a, j[k], b, j[k], abs(v[k]), int(got.regulator[-1]), int(got.target[-1])))
    assert same(got, select_ref(M, top=k + 1))
    assert (int(got.regulator[-1]), int(got.target[-1])) == (a, int(j[k]))


# --------------------------------------------------------------------------- 4. the refinement of a full cut bin
def test_a_full_cut_bin_is_refined_on_the_next_bits(pa, dev):
    from phoenix_amd import engine
    from phoenix_amd.odenet import params_of
    net, yd, mats = matrices(pa, dev, 200, 200, 2)
    params = engine.params_cached(*params_of(net))
    s = yd - 0.5
    ph = torch.exp(torch.addmm(params.bp, torch.log1p(s / (1 + s.abs())), params.Wp.t()))
    for mode, orient in (("effects", True), ("mean_abs", False)):
        M = mats[mode]
        bins = np.bincount(np.abs(select_ref(M, threshold=TINY, orient=orient)[2]).view(np.uint32) >> 19)
        assert bins.max() > 64                            # level-0 bins are fuller than the cap used below
        for sel in (dict(top=2000), dict(threshold=float(np.median(np.abs(M))))):
            got = pa.Edges(*engine.effects_edges(params, mode, y=yd, ph=ph, orient=orient, refine_above=64, **sel))
            ref = select_ref(M, orient=orient, **sel)
            print("%s orient=%d %s with the cut bin capped at 64 entries: %d edges" % (mode, orient, sel, len(ref[2])))
            assert len(ref[2]) >= 2000 and same(got, ref)


# --------------------------------------------------------------------------- 5. genome scale
def test_genome_shape_against_selection_by_torch(pa, dev):
    """N = 11 165, H = 40: the 50 000 strongest oriented edges against the same selection made by torch on the device from
    the dense matrix (key = inverted magnitude bits, then i N + j, as the semantics order the edges)"""
    N, H, K = 11165, 40, 50000
    _, net, _, _, _, _ = case(pa, dev, N, H, 1)
    got = pa.effects_edges(net, top=K, orient=True)
    M = pa.effects_matrix(net)
    mag = M.abs()
    ok = torch.isfinite(M) & (M != 0) & (mag > mag.t())
    key = ((0x7FFFFFFF - mag.view(torch.int32).to(torch.int64)) << 32) | torch.arange(N * N, device=dev).reshape(N, N)
    key = torch.where(ok, key, torch.full_like(key, 2 ** 63 - 1)).reshape(-1)
    best = torch.topk(key, K, largest=False, sorted=True).values
    flat = best & 0xFFFFFFFF
    print("N=%d: %d eligible entries, weakest of the %d edges %.4e" % (N, int(ok.sum()), K, float(got.value[-1].abs())))
    assert int(ok.sum()) > K and len(got.value) == K
    assert torch.equal(got.regulator, flat // N) and torch.equal(got.target, flat % N)
    assert torch.equal(got.value.view(torch.int32), M.reshape(-1)[flat].view(torch.int32))


# --------------------------------------------------------------------------- 6. no N x N buffer
def test_the_matrix_is_never_allocated(pa, dev):
    """N = 3000, H = 8, top = 1000: the matrix would be 36 MB.  The call owns a 16 KiB histogram (cached), the candidate
    list (12 bytes per candidate: the 1000 edges plus the rest of their 1/16-octave cut bin, a few thousand entries), the
    sort's keys, order and scratch (a few times the list) and the three results: well under 1 MB, budget 4 MB"""
    N, H, K = 3000, 8, 1000
    _, net, _, _, yd, _ = case(pa, dev, N, H, 2)
    for kw in (dict(), dict(orient=True), dict(y=yd, orient=True)):
        first = pa.effects_edges(net, top=K, **kw)          # steady state: parameter layout, workspace, library handles
        torch.cuda.synchronize()
        assert len(first.value) == K
        del first
        torch.cuda.empty_cache()
        torch.cuda.reset_peak_memory_stats()
        base = torch.cuda.memory_allocated()
        res = pa.effects_edges(net, top=K, **kw)
        torch.cuda.synchronize()
        grown = torch.cuda.max_memory_allocated() - base
        del res
        print("peak growth of effects_edges(top=%d, %s) at N=%d: %d bytes (the matrix: %d, budget 4 000 000)"
              % (K, sorted(kw), N, grown, 4 * N * N))
        assert grown < 4_000_000
