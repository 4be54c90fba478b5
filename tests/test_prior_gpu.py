"""Row f1: the two prior SpMM kernels, k_prior_spmm_sell<RT> for RT = 1..4 and the plain CSC
k_prior_spmm (csrc/phx_prior.inc), held element by element to the float64 product at the shapes where they take another
path: fewer rows than a row tile, a row tail, the grid-stride loops, both sides of every RT boundary, the LDS fallback
of `prior_targets`, and column structures with an empty slice, an almost-all-padding slice and a partial last slice
(tests/test_prior_cpu.py: synthetic_prior).  Run with `-m gpu`.

Reference: ref[:, j] = sum_e float64(X[:, row_e]) * float64(val_e) over the de-duplicated triplets.
Bar (derived, not measured): both kernels form an output as a left-to-right fp32 sum of the w_j products of its column,
in ascending row order, fused or not.  Every product rounds once and every one of the w_j - 1 additions once (u = 2^-24
each; the first addition, to 0, is exact), so no term is rounded more than w_j times and
|got - ref| <= g sum|x v| with g = w u / (1 - w u) <= (w + 2) u as long as w^2 u <= 2, i.e. w <= 5792 (asserted); the
slack of about 2 u also covers the float64 reference's own rounding (w 2^-53).  Outputs of empty columns are exactly 0.
A dropped, doubled or misplaced entry changes an output by a whole term, orders of magnitude above the bar."""
import functools

import numpy as np
import pytest
import torch

from test_prior_cpu import synthetic_prior

pytestmark = pytest.mark.gpu

# csrc/phx_host.hpp: `constexpr size_t LDS_BUDGET = 163840 - 1024;`  phx_prior_targets_sell (phx_engine.hip) stages
# RT = min(4, LDS_BUDGET / (4 N)) rows of X and refuses RT = 0.  The sizes below are derived from that budget: if it
# changes, `expected_rt` no longer matches the RT a case is there for and the case fails instead of losing coverage.
LDS_BUDGET = 163840 - 1024
ROW_FLOATS = LDS_BUDGET // 4                      # 40 704: the longest row of X one workgroup can stage
PHX_OK, PHX_ERR_BAD_ARG = 0, 4
CSC_GRID_ROWS = 2048                              # phx_prior_targets: gridDim.y = min(K, 2048)


def expected_rt(N):
    return min(4, LDS_BUDGET // (4 * N))


def rt_boundaries():
    """(N, RT) on both sides of 4|3, 3|2, 2|1 and the last N that fits"""
    out = []
    for rt in (4, 3, 2):
        n = ROW_FLOATS // rt                      # the largest N with RT = rt
        out += [(n, rt), (n + 1, rt - 1)]
    return out + [(ROW_FLOATS, 1)]


def test_rt_boundaries_are_those_of_the_lds_budget():
    assert rt_boundaries() == [(10176, 4), (10177, 3), (13568, 3), (13569, 2), (20352, 2), (20353, 1), (40704, 1)]
    assert all(expected_rt(n) == rt for n, rt in rt_boundaries())
    assert expected_rt(ROW_FLOATS + 1) == 0 and expected_rt(14691) == 2 and expected_rt(11165) == 3


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "these tests need the MI355X"
    return torch.device("cuda:0")


@functools.lru_cache(maxsize=2)
def case(N):
    """the synthetic prior of size N on the device and, per column, what the reference needs"""
    from phoenix_amd.prior import PriorMatrix
    rows, cols, vals, info = synthetic_prior(N)
    P = PriorMatrix(rows, cols, vals, N, "cuda:0")
    r, c, v = info["dedup"]
    assert P.nnz == len(v)
    return P, r, c, v.astype(np.float64), info


def reference(X, N, r, c, v):
    """(ref, sum |x v|) in float64, [K, N] each"""
    X = X.astype(np.float64)
    if N <= 2000:
        D = np.zeros((N, N), np.float64)
        D[r, c] = v
        return X @ D, np.abs(X) @ np.abs(D)
    ref, mag = np.empty_like(X), np.empty_like(X)
    for k in range(X.shape[0]):                   # a gather per entry, summed per column; no N x N array
        prod = X[k, r] * v
        ref[k] = np.bincount(c, weights=prod, minlength=N)
        mag[k] = np.bincount(c, weights=np.abs(prod), minlength=N)
    return ref, mag


def draw_x(K, N, seed):
    return np.random.RandomState(seed).uniform(-0.5, 1.0, (K, N)).astype(np.float32)


def hold(tag, got, ref, mag, col_len):
    got = got.astype(np.float64)
    assert got.shape == ref.shape, (tag, got.shape, ref.shape)
    assert np.all(np.isfinite(got)), "%s: %d non-finite (unwritten?) outputs" % (tag, int((~np.isfinite(got)).sum()))
    assert col_len.max() <= 5792                                  # the range the bar is derived for
    bar = (col_len + 2.0) * 2.0 ** -24 * mag
    err = np.abs(got - ref)
    ratio = np.where(bar > 0, err / np.where(bar > 0, bar, 1.0), np.where(err > 0, np.inf, 0.0))
    worst = np.unravel_index(np.argmax(ratio), err.shape)
    print("%s: K=%d N=%d max err %.3e, worst err/bar %.3f at row %d col %d (w=%d)"
          % (tag, ref.shape[0], ref.shape[1], err.max(), ratio[worst], worst[0], worst[1], col_len[worst[1]]))
    assert np.all(err <= bar), (tag, worst, got[worst], ref[worst], bar[worst])
    empty = col_len == 0
    assert empty.any() and np.all(got[:, empty] == 0), tag        # exactly 0, whatever the bar says


def run_sell(P, X, K, N):
    from phoenix_amd import _lib, engine
    out = torch.full_like(X, float("nan"))
    rc = _lib.load().phx_prior_targets_sell(engine._p(P.sell_ptr), engine._p(P.sell_width), engine._p(P.sell_rows),
                                            engine._p(P.sell_vals), engine._p(X), engine._p(out), K, N, engine._stream_ptr())
    return rc, out


def run_csc(P, X, K, N):
    from phoenix_amd import _lib, engine
    out = torch.full_like(X, float("nan"))
    rc = _lib.load().phx_prior_targets(engine._p(P.colptr), engine._p(P.rowidx), engine._p(P.vals), engine._p(X),
                                       engine._p(out), K, N, engine._stream_ptr())
    return rc, out


def check(dev, N, K, rt, entry_points=("prior_targets", "sell", "csc")):
    from phoenix_amd.prior import prior_targets
    assert expected_rt(N) == rt, "N = %d now gets RT = %d, this case is there for RT = %d" % (N, expected_rt(N), rt)
    P, r, c, v, info = case(N)
    Xh = draw_x(K, N, seed=K + N)
    ref, mag = reference(Xh, N, r, c, v)
    X = torch.from_numpy(Xh).to(dev)
    tag = "N=%d K=%d RT=%d" % (N, K, rt)
    if "prior_targets" in entry_points:
        got = prior_targets(X.reshape(K, 1, N), P)                 # [K,1,N], as the drivers pass it
        assert got.shape == (K, 1, N)
        hold(tag + " prior_targets", got.reshape(K, N).cpu().numpy(), ref, mag, info["col_len"])
    if "sell" in entry_points:
        rc, out = run_sell(P, X, K, N)
        if rt == 0:                                                # refused before anything is launched
            torch.cuda.synchronize()
            assert rc == PHX_ERR_BAD_ARG and bool(torch.isnan(out).all())
        else:
            assert rc == PHX_OK
            hold(tag + " sell", out.cpu().numpy(), ref, mag, info["col_len"])
    if "csc" in entry_points:
        rc, out = run_csc(P, X, K, N)
        assert rc == PHX_OK
        hold(tag + " csc", out.cpu().numpy(), ref, mag, info["col_len"])


@pytest.mark.parametrize("K", [1, 2, 3, 5, 9])
@pytest.mark.parametrize("N", [40, 64, 130])
def test_sub_slice_exact_slice_and_partial_slice(dev, N, K):
    """N < 64, N = 64 and N % 64 = 2 with RT = 4: K < RT and K % RT = 1, 2, 3 -- the rows `min(k0 + r, K - 1)` stages
    twice and `k0 + r < K` must not store"""
    check(dev, N, K, 4)


@pytest.mark.parametrize("N,rt", rt_boundaries())
def test_both_sides_of_every_rt_boundary(dev, N, rt):
    """k_prior_spmm_sell<4>, <3>, <2> and <1> at the largest and smallest N each is chosen for (RT = 2 is what the
    B-cell size N = 14 691 gets), K = 2 RT + 1: two full row tiles and a one-row tail"""
    check(dev, N, 2 * rt + 1, rt)


def test_lds_fallback_of_prior_targets(dev):
    """one gene more than a workgroup can stage: phx_prior_targets_sell returns PHX_ERR_BAD_ARG and launches nothing,
    `prior_targets` takes the plain CSC kernel"""
    check(dev, ROW_FLOATS + 1, 3, 0)


def test_grid_stride_loop_with_a_tail(dev):
    """one row tile more than the 4 * CUs workgroups of the sliced-ELL launch take in their first pass, plus one row:
    workgroup 0 runs `k0 += gridDim.x * RT` once and ends in a one-row tail"""
    from phoenix_amd import _lib
    rt = 4
    check(dev, 130, rt * 4 * _lib.load().phx_device_cus() + rt + 1, rt)


def test_csc_row_stride(dev):
    """k_prior_spmm: gridDim.y = min(K, 2048), so the rows from 2048 on are second iterations of `k += gridDim.y`"""
    check(dev, 130, CSC_GRID_ROWS + 37, 4, entry_points=("csc",))
