"""Row f1: prior-matrix parsing against the golden captured from the reference's
read_prior_matrix (CPU part; the SpMM itself is checked on the GPU in test_gpu_parity.py and test_prior_gpu.py), and the
CSC / sliced-ELL layouts of PriorMatrix against numpy restatements of the two kernels' walks."""
import os
import tempfile

import numpy as np
import pytest

from conftest import load_golden, sub


def _write_triplets(trip):
    fh = tempfile.NamedTemporaryFile("w", suffix=".csv", delete=False)
    for a, b, v in trip:
        fh.write("%d,%d,%g\n" % (a, b, v))
    fh.close()
    return fh.name


def test_triplet_format_matches_reference_dense():
    from phoenix_amd.prior import read_prior_matrix
    g = sub(load_golden("g8_prior"), "trip/")
    path = _write_triplets(g["triplets"])
    try:
        P = read_prior_matrix(path, sparse=True, num_genes=40, device="cpu")
    finally:
        os.unlink(path)
    assert np.array_equal(P.to_dense().numpy(), g["dense"])          # duplicates summed, 1-based indices
    assert np.array_equal(P.abs().to_dense().numpy(), np.abs(g["dense"]))


def test_dense_format_matches_reference():
    from phoenix_amd.prior import read_prior_matrix
    g = sub(load_golden("g8_prior"), "g350/")
    n = 350
    dense = np.zeros((n, n), np.float32)
    dense[g["rows"], g["cols"]] = g["vals"]
    fh = tempfile.NamedTemporaryFile("w", suffix=".csv", delete=False)
    np.savetxt(fh, dense, delimiter=",", fmt="%g")
    fh.close()
    try:
        P = read_prior_matrix(fh.name, sparse=False, device="cpu")
    finally:
        os.unlink(fh.name)
    assert P.N == n and P.nnz == len(g["vals"]) == 550               # 550 nnz of 122 500
    assert np.array_equal(P.to_dense().numpy(), dense)


# --------------------------------------------------------------------------- synthetic priors that stress the column structure
# (shared with tests/test_prior_gpu.py)
LONG = 300   # entries of the long column


def dedup_triplets(rows, cols, vals, N):
    """what `torch.sparse_coo_tensor(...).to_dense()` keeps of 0-based triplets (train_insilico.py:71-72): duplicates
    summed in float32, and no explicit zero; sorted by (col, row).  Stated with np.unique / np.add.at, independently of
    PriorMatrix's lexsort / reduceat."""
    keep = vals != 0
    key, inv = np.unique(cols[keep].astype(np.int64) * N + rows[keep], return_inverse=True)
    v = np.zeros(len(key), np.float32)
    np.add.at(v, inv, vals[keep].astype(np.float32))
    return key % N, key // N, v


def synthetic_prior(N, seed=0):
    """Seeded 0-based triplets (rows, cols, vals) with N(0, 1) values -- products with X are inexact -- and, beside a
    background of about 0.3 % density: an all-empty 64-column slice, a slice whose only non-empty column has LONG entries
    (a slice that is almost all padding), entries at (N-1, N-1) and (0, N-1), three duplicated coordinates (they are
    summed; one of them is (N-1, N-1)) and one explicit zero (it is dropped; it sits in the empty slice, which must stay
    empty).  The last slice holds column N-1, so an empty slice and a slice for the long column alone need three
    slices: with fewer (N <= 128) the long column shares slice 0 with the background and no slice is empty; a column
    holds at most N entries, so below N = LONG the long column is a full one.  Returns the triplets in arbitrary order
    and a dict of what was placed where; every property is asserted on the de-duplicated pattern."""
    rs = np.random.RandomState(1000 + 7 * seed + N % 997)
    three = (N + 63) // 64 >= 3
    long_len, long_col = min(LONG, N), (64 + 17 if three else 1)
    first_bg = 128 if three else 0                      # slice 0 stays empty, slice 1 holds the long column alone
    nbg = max(6, int(round(0.003 * N * N)))
    bg = np.unique(rs.randint(first_bg, N, nbg).astype(np.int64) * N + rs.randint(0, N, nbg))
    key = np.union1d(bg, np.concatenate([long_col * N + rs.permutation(N)[:long_len].astype(np.int64),
                                         [(N - 1) * N + N - 1, (N - 1) * N + 0]]))
    rows, cols = key % N, key // N
    vals = rs.randn(len(key)).astype(np.float32)
    vals[vals == 0] = 1.0
    dup = bg[rs.choice(len(bg), 2, replace=False)]                 # duplicated: two of the background and (N-1, N-1)
    dup_r, dup_c = (dup % N).tolist() + [N - 1], (dup // N).tolist() + [N - 1]
    zero_at = (N // 2, 5)                               # the explicit zero: in the empty slice if there is one
    while zero_at[1] * N + zero_at[0] in key:
        zero_at = (zero_at[0] - 1, 5)
    order = rs.permutation(len(key) + 4)                # file order is arbitrary
    rows = np.concatenate([rows, dup_r, [zero_at[0]]])[order]
    cols = np.concatenate([cols, dup_c, [zero_at[1]]])[order]
    vals = np.concatenate([vals, rs.randn(3).astype(np.float32) + 3.0, np.zeros(1, np.float32)])[order]
    # ---- the properties, on the de-duplicated pattern
    r, c, v = dedup_triplets(rows, cols, vals, N)
    lens = np.bincount(c, minlength=N)
    assert len(vals) - len(v) == 4 and int((vals == 0).sum()) == 1           # 3 duplicates summed, 1 zero dropped
    assert np.all(v != 0)
    assert 0.002 < len(bg) / float(N * N) < 0.0045                           # the background
    assert lens[long_col] == long_len == lens.max() and (long_len == LONG or N < LONG)
    kept = c * N + r
    assert (N - 1) * N + N - 1 in kept and (N - 1) * N + 0 in kept and zero_at[1] * N + zero_at[0] not in kept
    if three:
        assert lens[:64].sum() == 0 and zero_at[1] < 64                      # the all-empty slice, zero and all
        assert lens[64:128].sum() == long_len                                # the long column is alone in its slice
    return rows, cols, vals, {"three": three, "long_col": long_col, "long_len": long_len, "col_len": lens, "dedup": (r, c, v)}


def dense64(rows, cols, vals, N):
    r, c, v = dedup_triplets(rows, cols, vals, N)
    D = np.zeros((N, N), np.float64)
    D[r, c] = v
    return D


def product_in_row_order(X, D):
    """X @ D in fp64 with every output summed over the rows of D in ascending order (no BLAS blocking), so that a walk of
    a sparse layout in the same order reproduces it bit for bit: the zero terms do not change a sum"""
    acc = np.zeros((X.shape[0], D.shape[1]), np.float64)
    for r in range(D.shape[0]):
        acc += X[:, r:r + 1] * D[r:r + 1, :]
    return acc


def sell_walk(P, X):
    """numpy restatement of k_prior_spmm_sell's walk (csrc/phx_prior.inc) in fp64: slice s, lane l, i < width[s] reads
    sptr[s] + 64 i + l; returns all 64 * nslices columns, padded ones included"""
    sptr, width = P.sell_ptr.numpy(), P.sell_width.numpy()
    ridx, vals = P.sell_rows.numpy(), P.sell_vals.numpy().astype(np.float64)
    lanes = np.arange(64)
    acc = np.zeros((X.shape[0], 64 * len(width)), np.float64)
    for s in range(len(width)):
        for i in range(width[s]):
            at = sptr[s] + 64 * i + lanes
            acc[:, 64 * s:64 * s + 64] += X[:, ridx[at]] * vals[at]
    return acc


def csc_walk(P, X):
    """numpy restatement of k_prior_spmm's walk in fp64"""
    colptr, rowidx, vals = P.colptr.numpy(), P.rowidx.numpy(), P.vals.numpy().astype(np.float64)
    acc = np.zeros((X.shape[0], P.N), np.float64)
    for j in range(P.N):
        for e in range(colptr[j], colptr[j + 1]):
            acc[:, j] += X[:, rowidx[e]] * vals[e]
    return acc


@pytest.mark.parametrize("N", [40, 64, 130, 1000])
def test_sell_and_csc_layouts_reproduce_the_dense_product(N):
    """PriorMatrix._build_sell (padding, empty slices, the last partial slice) and the CSC arrays, without a GPU: the
    kernels' walks restated in numpy reproduce the fp64 dense product of the triplets exactly, and the layout
    invariants the kernels rely on hold."""
    from phoenix_amd.prior import PriorMatrix
    rows, cols, vals, info = synthetic_prior(N)
    P = PriorMatrix(rows, cols, vals, N, "cpu")
    D = dense64(rows, cols, vals, N)
    assert np.array_equal(P.to_dense().numpy().astype(np.float64), D) and P.nnz == np.count_nonzero(D)
    X = np.random.RandomState(N).uniform(-0.5, 1.0, (5, N)).astype(np.float32).astype(np.float64)
    ref = product_in_row_order(X, D)
    got = sell_walk(P, X)
    assert np.array_equal(got[:, :N], ref) and np.all(got[:, N:] == 0)
    assert np.array_equal(csc_walk(P, X), ref)
    assert np.all(ref[:, info["col_len"] == 0] == 0) and np.any(info["col_len"] == 0)
    # ---- layout invariants
    colptr, rowidx = P.colptr.numpy().astype(np.int64), P.rowidx.numpy()
    sptr, width = P.sell_ptr.numpy(), P.sell_width.numpy()
    ridx, sv = P.sell_rows.numpy(), P.sell_vals.numpy()
    ns = (N + 63) // 64
    lens = np.zeros(64 * ns, np.int64)
    lens[:N] = info["col_len"]
    assert np.array_equal(np.diff(colptr), info["col_len"]) and colptr[0] == 0 and colptr[-1] == P.nnz
    assert sptr.dtype == np.int64 and width.dtype == np.int32 and ridx.dtype == np.int32 and sv.dtype == np.float32
    assert len(width) == len(sptr) == ns and np.array_equal(width, lens.reshape(ns, 64).max(axis=1))
    assert np.array_equal(sptr, np.concatenate([[0], np.cumsum(64 * width.astype(np.int64))])[:-1])   # running sum
    assert len(ridx) == len(sv) == 64 * int(width.sum())
    if info["three"]:
        assert width[0] == 0 and sptr[1] == 0 and width[1] == info["long_len"]
    real = np.zeros(len(sv), bool)
    for j in range(N):
        at = sptr[j // 64] + 64 * np.arange(lens[j]) + j % 64
        real[at] = True
        col_rows = rowidx[colptr[j]:colptr[j + 1]]
        assert np.all(np.diff(col_rows) > 0)                                  # rows ascend inside a column
        assert np.array_equal(ridx[at], col_rows) and np.array_equal(sv[at], P.vals.numpy()[colptr[j]:colptr[j + 1]])
    assert real.sum() == P.nnz and np.all(sv[real] != 0)
    assert np.all(ridx[~real] == 0) and np.all(sv[~real] == 0) and not np.any(np.signbit(sv[~real]))   # padding: (row 0, +0)
    assert 0 <= ridx.min() and ridx.max() == N - 1 == rowidx.max()            # the last row is there
    # ---- abs() touches both value arrays, shares the index arrays and leaves the original alone
    A = P.abs()
    assert np.any(P.vals.numpy() < 0) and np.any(sv < 0)
    assert np.array_equal(A.vals.numpy(), np.abs(P.vals.numpy())) and np.array_equal(A.sell_vals.numpy(), np.abs(sv))
    assert A.sell_rows is P.sell_rows and A.rowidx is P.rowidx and A.sell_ptr is P.sell_ptr
    assert np.array_equal(sell_walk(A, X)[:, :N], product_in_row_order(X, np.abs(D)))
    assert np.array_equal(P.sell_vals.numpy(), sv) and np.array_equal(sell_walk(P, X)[:, :N], ref)
