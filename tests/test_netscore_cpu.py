"""CPU-only checks of the network-scoring boundary (phx_effects_gather / phx_effects_rank_counts /
phx_effects_rank_workspace_bytes, include/phoenix_hip.h; `read_network`, `effects_at`, `network_score`): `score_ref`, the numpy
restatement with integer counts that tests/test_netscore_gpu.py holds the kernels to, is pinned to the reference's own
ranking (get_link_list), masking (make_mask) and scoring (COMPUTE_GRN_AUROC's roc_auc_score, plus sklearn's
average_precision_score and curve points) through the fixture g22_netscore.npz (tests/golden/make_golden_netscore.py);
`read_network` parses the fixture's files; the symbols exist, the argument checks answer before any device call, and the
Python callers refuse bad arguments and a CPU network."""
import collections
import ctypes as C

import numpy as np
import pytest
import torch

from conftest import load_golden
from test_abi_cpu import _declared_symbols

BAD_ARG, WORKSPACE = 4, 5
ORIENT, DIAGONAL = 1, 2
WS_BYTES = 64

Score = collections.namedtuple("Score", ("auroc", "average_precision", "n_positive", "n_negative", "threshold", "tp", "fp"))


def mask_ref(M):
    """make_mask (extract_model_matrix_PHOENIX.py:29-37) as a copy: an entry keeps its value only when |M[i,j]| > |M[j,i]|
    (false with a NaN on either side); everything else, the diagonal included, is +0"""
    M = np.asarray(M)
    with np.errstate(invalid="ignore"):
        keep = np.abs(M) > np.abs(M.T)
    return np.where(keep, M, np.float32(0)).astype(np.float32)


def score_ref(M, regulator, target, orient=False, diagonal=False):
    """Score(auroc, average_precision, n_positive, n_negative, threshold float32 [m] descending, tp int64 [m], fp int64 [m])
    of the float32 matrix M [N, N] (regulator row, target column) against the label pairs: the score of an entry is its
    magnitude bits (`orient`: of mask_ref(M)), scored are the off-diagonal entries (`diagonal`: all), positives are the
    distinct label pairs among them, everything else is a negative.  Integer counts throughout; the two scores are
        U2 = sum over all scored entries of (2 #positives above it + #positives equal to it) - P^2,  AUROC = U2 / (2 P Nn)
        AP = sum_k (tp[k] - tp[k-1]) / P * tp[k] / (tp[k] + fp[k])
    ValueError for labels of one class and for a scored entry that is not finite."""
    M = np.asarray(M)
    assert M.dtype == np.float32 and M.ndim == 2 and M.shape[0] == M.shape[1]
    N = M.shape[0]
    X = mask_ref(M) if orient else M
    mag = (X.view(np.uint32) & np.uint32(0x7FFFFFFF)).astype(np.int64)
    scored = np.ones((N, N), bool) if diagonal else ~np.eye(N, dtype=bool)
    label = np.zeros((N, N), bool)
    label[np.asarray(regulator, np.int64), np.asarray(target, np.int64)] = True
    label &= scored
    P, Nn = int(label.sum()), int(scored.sum() - label.sum())
    if P == 0 or Nn == 0:
        raise ValueError("Only one class present")
    bad = int((mag[scored] >= 0x7F800000).sum())
    if bad:
        raise ValueError("%d scored entries are not finite" % bad)
    u, mult = np.unique(mag[label], return_counts=True)              # ascending
    x = mag[scored]
    lb = np.searchsorted(u, x, side="left")
    eq = (lb < len(u)) & (u[np.minimum(lb, len(u) - 1)] == x)
    ge_pos = np.cumsum(mult[::-1])[::-1]                              # positives >= u[k]
    ge_pos_ext = np.append(ge_pos, 0)
    gt = np.where(eq, ge_pos_ext[np.minimum(lb + 1, len(u))], ge_pos_ext[lb])
    U2 = int((2 * gt + np.where(eq, mult[np.minimum(lb, len(u) - 1)], 0)).sum()) - P * P
    ge_all = (len(x) - np.searchsorted(np.sort(x), u[::-1], side="left")).astype(np.int64)     # scored entries >= u[k]
    tp = ge_pos[::-1].astype(np.int64)
    fp = ge_all - tp
    hits = mult[::-1].astype(np.float64)
    ap = float((hits / P * (tp.astype(np.float64) / (tp + fp).astype(np.float64))).sum())
    return Score(U2 / (2 * P * Nn), ap, P, Nn, u[::-1].astype(np.uint32).view(np.float32), tp, fp)


def _lib():
    from phoenix_amd import _lib
    return _lib, _lib.load()


# --------------------------------------------------------------------------- the restatement against the reference
def test_mask_ref_is_the_reference_make_mask():
    g = load_golden("g22_netscore")
    got = mask_ref(g["matrix"])
    assert np.array_equal(got.view(np.uint32), g["masked"].view(np.uint32))
    assert np.all(np.diag(got) == 0)
    n = np.float32(np.nan)
    M = np.array([[1, n, 2], [3, 5, -2], [-4, n, 0]], np.float32)
    assert np.array_equal(mask_ref(M), np.array([[0, 0, 0], [0, 0, 0], [-4, 0, 0]], np.float32))     # NaN loses both ways


@pytest.mark.parametrize("tag,orient", [("plain", False), ("orient", True)])
def test_score_ref_reproduces_the_reference_scores_and_sklearns_curves(tag, orient):
    g = load_golden("g22_netscore")
    s = score_ref(g["matrix"], g["regulator"], g["target"], orient=orient)
    auroc, ap = float(g[tag + "_auroc"]), float(g[tag + "_ap"])
    print("G22 %s: AUROC %.15f (reference %.15f), AP %.15f (sklearn %.15f), %d positives at %d distinct magnitudes, %d negatives"
          % (tag, s.auroc, auroc, s.average_precision, ap, s.n_positive, len(s.threshold), s.n_negative))
    assert (s.n_positive, s.n_negative) == (int(g[tag + "_n_pos"]), int(g[tag + "_n_neg"]))
    assert abs(s.auroc - auroc) <= 1e-12 * abs(auroc) and abs(s.average_precision - ap) <= 1e-12 * abs(ap)
    # the curve points: sklearn lists every distinct score; ours are those of them that a positive has
    thr, tp, fp = g[tag + "_roc_thr"], g[tag + "_roc_tp"], g[tag + "_roc_fp"]
    at = {float(t): k for k, t in enumerate(thr)}
    idx = np.array([at[float(t)] for t in s.threshold])
    assert np.all(np.diff(s.threshold) < 0) and len(s.threshold) > 5
    assert np.array_equal(s.tp, tp[idx]) and np.array_equal(s.fp, fp[idx])
    assert set(np.nonzero(np.diff(np.concatenate([[0], tp])))[0].tolist()) == set(idx.tolist())   # no bend is missed
    pthr, prec, rec = g[tag + "_pr_thr"], g[tag + "_pr_precision"], g[tag + "_pr_recall"]
    pat = {float(t): k for k, t in enumerate(pthr)}
    pidx = np.array([pat[float(t)] for t in s.threshold])
    assert np.allclose(s.tp / (s.tp + s.fp), prec[pidx], rtol=1e-12, atol=0)
    assert np.allclose(s.tp / s.n_positive, rec[pidx], rtol=1e-12, atol=0)


def test_golden_is_what_its_generator_asserts():
    g = load_golden("g22_netscore")
    M, r, t = g["matrix"], g["regulator"], g["target"]
    assert M.dtype == np.float32 and M.shape == (200, 200) and len(r) == len(t) == 484
    assert len(set(r.tolist())) == 5 and int((r == t).sum()) == 4          # few regulators; the self-edges are kept
    assert np.all(M[:, [17, 140]] == 0) and 0.25 < float((M == 0).mean()) < 0.35 and (M < 0).any()
    off = r != t
    assert float(np.abs(M[r[off], t[off]]).max()) == float(np.abs(M).max()) == 3.0 and int((np.abs(M) == 3.0).sum()) == 1
    assert len(np.unique(np.abs(M))) < 100                      # ties abound
    # `diagonal` admits the self-edges of the network and nothing else changes class
    a, b = score_ref(M, r, t), score_ref(M, r, t, diagonal=True)
    assert b.n_positive == a.n_positive + int((~off).sum()) and b.n_positive + b.n_negative == 200 * 200


def test_score_ref_on_a_matrix_small_enough_to_count_by_hand():
    M = np.array([[9.0, 2.0, -2.0, 0.0],
                  [2.0, 0.0, 3.0, 5.0],
                  [1.0, -3.0, -0.0, 0.0],
                  [4.0, 5.0, 7.0, 8.0]], np.float32)
    # positives (0,1) = 2, (3,2) = 7, (2,3) = 0, and a duplicate and a self-edge that do not count
    s = score_ref(M, [0, 3, 2, 0, 1], [1, 2, 3, 1, 1])
    assert (s.n_positive, s.n_negative) == (3, 9)
    assert s.threshold.tolist() == [7.0, 2.0, 0.0] and s.tp.tolist() == [1, 2, 3] and s.fp.tolist() == [0, 7, 9]
    # negatives: 0, 5, 5, 4, 3, 3, 2, 2, 1 ; pairs won: 7 beats 9, 2 beats 0 and 1 and ties twice, 0 ties once
    assert s.auroc == (9 + 2 + 0.5 * 2 + 0.5 * 1) / 27
    assert s.average_precision == pytest.approx(1 / 3 * (1 / 1) + 1 / 3 * (2 / 9) + 1 / 3 * (3 / 12), rel=1e-15)
    d = score_ref(M, [0, 3, 2, 0, 1], [1, 2, 3, 1, 1], diagonal=True)
    assert (d.n_positive, d.n_negative) == (4, 12) and d.threshold.tolist() == [7.0, 2.0, 0.0] and d.tp.tolist() == [1, 2, 4]
    # orient: (0,1)/(1,0) tie -> both 0; (3,2) beats (2,3)
    o = score_ref(M, [0, 3, 2], [1, 2, 3], orient=True)
    assert o.threshold.tolist() == [7.0, 0.0] and o.tp.tolist() == [1, 3]
    # the only negative-free threshold is 7; the other two positives, (0,1) tied and (2,3) the weaker, score 0
    assert o.fp.tolist() == [0, 9]
    for labels in (([], []), ([1], [1])):
        with pytest.raises(ValueError, match="Only one class present"):
            score_ref(M, *labels)
    i, j = np.nonzero(~np.eye(4, dtype=bool))
    with pytest.raises(ValueError, match="Only one class present"):
        score_ref(M, i, j)
    M[1, 2] = np.inf
    with pytest.raises(ValueError, match="1 scored entries are not finite"):
        score_ref(M, [0], [1])
    M[1, 2] = np.nan
    assert score_ref(M, [0], [2], orient=True).n_negative == 11          # make_mask turns a NaN and its partner into 0


# --------------------------------------------------------------------------- read_network
def _files(tmp_path):
    g = load_golden("g22_netscore")
    names, net = tmp_path / "names.csv", tmp_path / "network.csv"
    names.write_text(str(g["names_csv"]))
    net.write_text(str(g["network_csv"]))
    return g, str(names), str(net)


def test_read_network_gives_the_stored_index_pairs(tmp_path):
    import phoenix_amd
    g, names, net = _files(tmp_path)
    r, t = phoenix_amd.read_network(net, names)
    assert r.dtype == t.dtype == np.int64
    assert np.array_equal(r, g["regulator"]) and np.array_equal(t, g["target"])
    listed = [line for line in str(g["names_csv"]).splitlines()[1:]]
    r2, t2 = phoenix_amd.read_network(net, listed)
    assert np.array_equal(r2, r) and np.array_equal(t2, t)
    # fewer genes: the rows that name one of the others are dropped
    r3, t3 = phoenix_amd.read_network(net, listed[:120])
    keep = (r < 120) & (t < 120)
    assert 0 < keep.sum() < len(r) and np.array_equal(r3, r[keep]) and np.array_equal(t3, t[keep])


def test_read_network_drops_unknown_names_and_duplicates_and_ignores_further_columns(tmp_path):
    import phoenix_amd
    fp = tmp_path / "edge_properties.csv"
    fp.write_text('"from","to","weight","activation","EC50","n"\n'
                  '"C","A",1,FALSE,0.45,1.57\n'
                  '"A","B",1,TRUE,0.51,1.67\n'
                  '"C","A",1,TRUE,0.46,1.72\n'
                  '"A","nobody",1,TRUE,0.5,1.5\n'
                  'B,B,1,TRUE,0.5,1.5\n'
                  '"nobody","A",1,TRUE,0.5,1.5\n'
                  '"A","A"\n')
    r, t = phoenix_amd.read_network(str(fp), ["A", "B", "C"])
    assert list(zip(r.tolist(), t.tolist())) == [(0, 0), (0, 1), (1, 1), (2, 0)]
    r, t = phoenix_amd.read_network(str(fp), ["Z"])
    assert r.shape == t.shape == (0,) and r.dtype == t.dtype == np.int64


# --------------------------------------------------------------------------- the C boundary
def test_the_symbols_are_exported_and_declared():
    mod, lib = _lib()
    for name in ("phx_effects_rank_workspace_bytes", "phx_effects_gather", "phx_effects_rank_counts"):
        assert name in mod.EXPORTS and name in _declared_symbols() and hasattr(lib, name), name
    assert set(mod.EXPORTS) == set(_declared_symbols())
    assert lib.phx_abi_version() == 7       # an additive change
    import phoenix_amd
    for name in ("read_network", "effects_at", "network_score", "NetworkScore"):
        assert getattr(phoenix_amd, name) is getattr(phoenix_amd.analysis, name)
    assert phoenix_amd.NetworkScore._fields == Score._fields


def _params(mod, N=8, H=3, **null):
    """phx_params with made-up device addresses"""
    addr = {"Ws": 0x1000, "bs": 0x2000, "Wp": 0x3000, "bp": 0x4000, "WaT": 0x5000, "g": 0x6000}
    addr.update(null)
    return mod.PhxParams(addr["Ws"], addr["bs"], addr["Wp"], addr["bp"], addr["WaT"], addr["g"], N, H, None)


def _gather(mod, lib, p="default", mode=2, y=0x7000, ph=0x8000, B=3, flags=ORIENT, keys=0x9000, offsets=0xa000, n=16,
            values=0xb000):
    if p == "default":
        p = _params(mod)
    return lib.phx_effects_gather(None if p is None else C.byref(p), mode, y, ph, B, flags, keys, offsets, n, values, None)


def _rank(mod, lib, p="default", mode=2, y=0x7000, ph=0x8000, B=3, flags=ORIENT, u=0x9000, m=16, counts=0xa000, ws=0xb000,
          ws_bytes=WS_BYTES):
    if p == "default":
        p = _params(mod)
    return lib.phx_effects_rank_counts(None if p is None else C.byref(p), mode, y, ph, B, flags, u, m, counts, ws, ws_bytes,
                                       None)


def test_bad_arguments_are_rejected_without_a_gpu():
    """only calls that must return before touching the device"""
    mod, lib = _lib()
    for call in (_gather, _rank):
        assert call(mod, lib, p=None) == BAD_ARG
        for name in ("Ws", "Wp", "WaT", "g"):
            assert call(mod, lib, p=_params(mod, **{name: None})) == BAD_ARG, name
        for bad in (dict(N=1), dict(N=0), dict(N=-8), dict(N=65536), dict(N=70000), dict(H=0), dict(H=257), dict(H=-1)):
            assert call(mod, lib, p=_params(mod, **bad)) == BAD_ARG, bad
        for mode in (-1, 3, 7):
            assert call(mod, lib, mode=mode) == BAD_ARG, mode
        for mode in (1, 2):                                    # the Jacobian modes need their states
            for bad in (dict(y=None), dict(ph=None), dict(B=0), dict(B=-2)):
                assert call(mod, lib, mode=mode, **bad) == BAD_ARG, bad
        for flags in (-1, 4, 8, 7):
            assert call(mod, lib, flags=flags) == BAD_ARG, flags
    for bad in (dict(keys=None), dict(offsets=None), dict(values=None), dict(n=0)):
        assert _gather(mod, lib, **bad) == BAD_ARG, bad
    for bad in (dict(u=None), dict(counts=None), dict(m=0), dict(m=2 ** 31), dict(m=2 ** 32 - 1)):
        assert _rank(mod, lib, **bad) == BAD_ARG, bad
    # every argument in order: the workspace is asked for next
    assert _rank(mod, lib, ws=None) == WORKSPACE
    assert _rank(mod, lib, ws_bytes=WS_BYTES - 1) == WORKSPACE
    assert _rank(mod, lib, mode=0, y=None, ph=None, B=0, flags=DIAGONAL, ws_bytes=0) == WORKSPACE


def test_workspace_bytes_is_zero_for_a_refused_shape():
    _, lib = _lib()
    f = lib.phx_effects_rank_workspace_bytes
    for shape in ((70000, 40, 3, 2), (1, 40, 3, 2), (0, 40, 3, 2), (-5, 40, 3, 2), (65536, 40, 3, 2), (350, 0, 3, 2),
                  (350, 257, 3, 2), (350, 40, 0, 2), (350, 40, 0, 1), (350, 40, 3, 5), (350, 40, 3, -1)):
        assert f(*shape) == 0, shape
    for shape in ((350, 40, 3, 2), (2, 1, 1, 1), (65535, 256, 1, 0), (350, 40, 0, 0), (350, 40, -7, 0)):   # effects ignores B
        assert f(*shape) == WS_BYTES, shape
    assert f.restype is C.c_size_t


# --------------------------------------------------------------------------- the Python callers
def test_python_callers_refuse_bad_arguments_and_a_cpu_network():
    import phoenix_amd
    net = phoenix_amd.ODENet("cpu", 16, neurons=4)
    y = torch.rand(3, 16)
    for fn in (phoenix_amd.effects_at, phoenix_amd.network_score):
        for r, t in (([0, 1, 2], [1, 2]), ([0, 16], [1, 2]), ([0, 1], [-1, 2]), (np.array([0, 1]), np.array([3, 99])),
                     ([0.5, 1.0], [1, 2]), ([[0, 1]], [[1, 2]]), (torch.tensor([0, 1]), torch.tensor([1]))):
            with pytest.raises(ValueError, match=fn.__name__):
                fn(net, r, t)
            with pytest.raises(ValueError, match=fn.__name__):
                fn(net, r, t, y=y, orient=True)
        for reduce in ("sum", "abs", None, "effects", 1):
            with pytest.raises(ValueError, match="reduce"):
                fn(net, [0, 1], [1, 2], y=y, reduce=reduce)
        for kw in (dict(), dict(orient=True), dict(y=y), dict(y=y, reduce="mean")):
            with pytest.raises(RuntimeError, match="must live on the GPU"):
                fn(net, [0, 1], [1, 2], **kw)
            with pytest.raises(RuntimeError, match="must live on the GPU"):
                fn(net, np.array([0, 1]), torch.tensor([1, 2]), **kw)
    with pytest.raises(RuntimeError, match="must live on the GPU"):
        phoenix_amd.network_score(net, [0], [1], diagonal=True)
