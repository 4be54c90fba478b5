"""Network scoring on the MI355X: `effects_at` and `network_score` (phx_effects_gather / phx_effects_rank_counts through
phoenix_amd.engine) against the matrix that `effects_matrix` / `jacobian_matrix` return, brought to the host, masked by
`mask_ref` for orient and scored by `score_ref` (tests/test_netscore_cpu.py, pinned there to the reference's make_mask and
get_link_list and to sklearn).  Neither is code under test.  The kernels promise the matrix's own bits and exact integer
counts, so the values, thresholds and counts are compared exactly; AUROC and average precision are the same float64
arithmetic on the same integers on both sides and are held to 1e-12 relative.  Shapes are those of tests/test_edges_gpu.py.
Every test prints what it measured before it asserts (run with -s to see it)."""
import numpy as np
import pytest
import torch

from conftest import load_golden
from test_edges_gpu import MODES, SHAPES, matrices
from test_effects_gpu import case
from test_gpu_parity import make_net, rand_params
from test_netscore_cpu import mask_ref, score_ref

pytestmark = pytest.mark.gpu

REL = 1e-12


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "these tests need the MI355X"
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def pa():
    import phoenix_amd
    return phoenix_amd


def calls(pa, net, yd, mode):
    kw = {} if mode == "effects" else dict(y=yd, reduce=mode)
    return (lambda r, t, **k: pa.effects_at(net, r, t, **kw, **k)), (lambda r, t, **k: pa.network_score(net, r, t, **kw, **k))


def label_sets(X, N, H):
    """{name: (regulator, target)} for the scored matrix X (masked already under orient)"""
    rng = np.random.default_rng(1000 * N + H)
    sets = {}
    # (a) about 2 N random pairs with self-edges, both directions of some pairs and duplicates
    r, t = rng.integers(0, N, 2 * N), rng.integers(0, N, 2 * N)
    r[:5], t[:5] = np.arange(5), np.arange(5)
    r[5:15], t[5:15] = t[20:30], r[20:30]
    r[15:20], t[15:20] = r[40:45], t[40:45]
    sets["a"] = (r, t)
    # (b) one positive
    sets["b"] = (np.array([N - 1]), np.array([N // 2]))
    # (c) every off-diagonal pair but one
    i, j = np.nonzero(~np.eye(N, dtype=bool))
    drop = (N * N) // 3
    sets["c"] = (np.delete(i, drop), np.delete(j, drop))
    # (d) positives from a zero column and from tie groups only
    mag = X.view(np.uint32) & np.uint32(0x7FFFFFFF)
    zero_cols = np.nonzero((mag == 0).all(axis=0))[0]
    assert len(zero_cols) >= 1
    vals, inverse, cnt = np.unique(mag, return_inverse=True, return_counts=True)
    tied = (cnt[inverse.reshape(N, N)] > 1) & ~np.eye(N, dtype=bool)
    ti, tj = np.nonzero(tied)
    pick = rng.permutation(len(ti))[:N]
    sets["d"] = (np.concatenate([np.arange(N)[::3], ti[pick]]), np.concatenate([np.full(len(range(0, N, 3)), zero_cols[0]), tj[pick]]))
    if N == 200:
        g = load_golden("g22_netscore")
        sets["e"] = (g["regulator"], g["target"])
    return sets


def same_score(got, ref):
    """(everything exact is exact, the two floats within REL)"""
    thr, tp, fp = got.threshold.cpu().numpy(), got.tp.cpu().numpy(), got.fp.cpu().numpy()
    exact = (got.threshold.dtype == torch.float32 and got.tp.dtype == got.fp.dtype == torch.int64 and
             got.threshold.is_cuda and got.tp.is_cuda and got.fp.is_cuda and
             isinstance(got.auroc, float) and isinstance(got.average_precision, float) and
             (got.n_positive, got.n_negative) == (ref.n_positive, ref.n_negative) and
             np.array_equal(thr.view(np.uint32), ref.threshold.view(np.uint32)) and
             np.array_equal(tp, ref.tp) and np.array_equal(fp, ref.fp))
    d_auc = abs(got.auroc - ref.auroc) / abs(ref.auroc) if ref.auroc else abs(got.auroc)
    d_ap = abs(got.average_precision - ref.average_precision) / abs(ref.average_precision)
    return exact, d_auc, d_ap


# --------------------------------------------------------------------------- 1. every shape, mode, flag and label set
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("N,H,B", SHAPES)
def test_values_and_scores_equal_score_ref_of_the_matrix(pa, dev, N, H, B, mode):
    net, yd, mats = matrices(pa, dev, N, H, B)
    M = mats[mode]
    at, score = calls(pa, net, yd, mode)
    for orient in (False, True):
        X = mask_ref(M) if orient else M
        sets = label_sets(X, N, H)
        for name, (r, t) in sets.items():
            v = at(r, t, orient=orient)
            assert v.dtype == torch.float32 and v.is_cuda and tuple(v.shape) == (len(r),)
            bits_ok = np.array_equal(v.cpu().numpy().view(np.uint32), X[r, t].view(np.uint32))
            report = []
            for diagonal in (False, True):
                ref = score_ref(M, r, t, orient=orient, diagonal=diagonal)
                got = score(r, t, orient=orient, diagonal=diagonal)
                exact, d_auc, d_ap = same_score(got, ref)
                report.append((diagonal, got.n_positive, len(got.threshold), got.auroc, got.average_precision, exact, d_auc, d_ap))
            print("N=%d H=%d B=%d %s orient=%d labels (%s) E=%d: value bits identical %s; (diagonal, positives, thresholds, "
                  "AUROC, AP, counts identical, rel. diff AUROC, AP) %s" % (N, H, B, mode, orient, name, len(r), bits_ok, report))
            assert bits_ok
            assert all(x[5] and x[6] <= REL and x[7] <= REL for x in report), report
            if name == "c" and not orient and N != 37:
                assert report[0][2] > (N * N) // 2, report[0][2]       # m is close to N^2: the deep end of the search


def test_index_tensors_on_the_device_and_an_empty_list(pa, dev):
    net, yd, mats = matrices(pa, dev, 97, 7, 5)
    M = mats["mean_abs"]
    r, t = label_sets(M, 97, 7)["a"]
    rd, td = torch.from_numpy(r).to(dev), torch.from_numpy(t).to(dev).to(torch.int32)
    v = pa.effects_at(net, rd, td, y=yd)
    assert np.array_equal(v.cpu().numpy().view(np.uint32), M[r, t].view(np.uint32))
    assert same_score(pa.network_score(net, rd, td, y=yd), score_ref(M, r, t))[0]
    e = pa.effects_at(net, [], [], y=yd)
    assert e.dtype == torch.float32 and e.is_cuda and e.numel() == 0


def test_two_runs_give_identical_results(pa, dev):
    net, yd, mats = matrices(pa, dev, 130, 40, 2)
    for mode in MODES:
        at, score = calls(pa, net, yd, mode)
        for orient in (False, True):
            r, t = label_sets(mask_ref(mats[mode]) if orient else mats[mode], 130, 40)["a"]
            a, b = score(r, t, orient=orient), score(r, t, orient=orient)
            assert len(a.threshold) > 100
            assert a[:4] == b[:4] and all(torch.equal(x, z) for x, z in zip(a[4:], b[4:])), (mode, orient)
            assert torch.equal(at(r, t, orient=orient).view(torch.int32), at(r, t, orient=orient).view(torch.int32))


# --------------------------------------------------------------------------- 2. the reference's network
def test_the_golden_network_on_the_golden_sized_model(pa, dev):
    """the ChIP sub-network of G22 against the (200, 200, 2) model: positives from 5 regulators, self-edges among them"""
    g = load_golden("g22_netscore")
    r, t = g["regulator"], g["target"]
    net, yd, mats = matrices(pa, dev, 200, 200, 2)
    for orient in (False, True):
        ref = score_ref(mats["effects"], r, t, orient=orient)
        got = pa.network_score(net, r, t, orient=orient)
        print("G22 network, effects, orient=%d: AUROC %.6f, AP %.6f, %d positives, %d negatives"
              % (orient, got.auroc, got.average_precision, got.n_positive, got.n_negative))
        assert got.n_positive == int((r != t).sum()) and got.n_positive + got.n_negative == 200 * 199
        exact, d_auc, d_ap = same_score(got, ref)
        assert exact and d_auc <= REL and d_ap <= REL


# --------------------------------------------------------------------------- 3. errors that need the device
def test_a_non_finite_scored_entry_is_an_error(pa, dev):
    """one NaN weight makes a regulator's whole row NaN: a value check, nothing faults"""
    N, H, B = 97, 7, 3
    p = rand_params(N, H, seed=17, std=0.6 / np.sqrt(N))
    p["Ws"][2, 40] = np.nan
    _, net, _, _, yd, _ = case(pa, dev, N, H, B, p=p)
    M = pa.effects_matrix(net).cpu().numpy()
    bad = int((~np.isfinite(M[~np.eye(N, dtype=bool)])).sum())
    print("NaN in Ws[2, 40]: %d off-diagonal entries of the effects matrix are not finite" % bad)
    assert bad == N - 1
    with pytest.raises(ValueError, match=r"\b%d scored entries are not finite" % bad):
        pa.network_score(net, [0, 1], [1, 2])
    with pytest.raises(ValueError, match=r"\b%d scored entries are not finite" % (bad + 1)):
        pa.network_score(net, [0, 1], [1, 2], diagonal=True)
    with pytest.raises(ValueError, match="not finite"):
        pa.network_score(net, [0, 1], [1, 2], y=yd)
    # make_mask turns a NaN and its partner into 0: the masked matrix is finite and is scored like any other
    ref = score_ref(M, [0, 1], [1, 2], orient=True)
    exact, d_auc, d_ap = same_score(pa.network_score(net, [0, 1], [1, 2], orient=True), ref)
    assert exact and d_auc <= REL and d_ap <= REL
    v = pa.effects_at(net, [40, 3, 40], [3, 40, 40])
    assert np.array_equal(v.cpu().numpy().view(np.uint32), M[[40, 3, 40], [3, 40, 40]].view(np.uint32))
    assert pa.effects_at(net, [40, 3], [3, 40], orient=True).cpu().numpy().view(np.uint32).tolist() == [0, 0]


def test_labels_of_one_class_are_an_error(pa, dev):
    N = 33
    net, yd, _ = matrices(pa, dev, N, 1, 1)
    i, j = np.nonzero(~np.eye(N, dtype=bool))
    for labels, kw in ((([], []), {}), (([3, 4], [3, 4]), {}), ((i, j), {}), ((i, j), dict(orient=True)),
                       ((np.repeat(np.arange(N), N), np.tile(np.arange(N), N)), dict(diagonal=True))):
        with pytest.raises(ValueError, match="Only one class present"):
            pa.network_score(net, *labels, **kw)
        with pytest.raises(ValueError, match="Only one class present"):
            pa.network_score(net, *labels, y=yd, **kw)
    assert pa.network_score(net, i, j, diagonal=True).n_negative == N        # the diagonal is the other class


def test_a_host_state_is_refused(pa, dev):
    net, yd, _ = matrices(pa, dev, 33, 1, 1)
    for fn in (pa.effects_at, pa.network_score):
        with pytest.raises(RuntimeError, match="must live on the GPU"):
            fn(net, [0], [1], y=yd.cpu())
