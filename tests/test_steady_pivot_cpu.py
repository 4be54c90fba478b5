"""CPU-only: the inputs, the truth and the bars of tests/test_steady_pivot_gpu.py, which holds the two dense solves of the
steady-state family -- k_st_solve (phx_steady_solve, (I - S) x = w) and k_sr_inverse (phx_steady_inverse, Z = (I - S)^-1), both
LU with partial pivoting in double, one workgroup of sixteen waves per state, n = 2H <= 512 -- to float64 on systems that
exchange rows, and the proof that those bars bite.

Why: at the float64 fixed points of the test models (tests/test_steady_cpu.py, N <= 600, m = 1 on the moving genes) scipy's
lu_factor of I - S, the same pivot rule, exchanges no row in any state with n >= 128, in I - S or in its transpose; only
(97, 7) at n = 14 (2 exchanges in three of five states) and (96, 56) at n = 112 (1 in one of four states, 3 in its transpose)
exchange at all, max |S| is 0.15 .. 1.2, and the only other solve inputs of the suite are 4 x 4 diagonal matrices.  So the row
swap, the swap of the right-hand side, the pivot search over more than one wave, the cross-wave reduction and the late info
codes had in effect never run under a test.

The mirror (`mirror`) is a float64 numpy LU that follows the rule as the kernels' comments state it: the pivot is the largest
|A[i][k]| over i >= k, the first i among equals (found per wave of 64 candidates i = k + 64 v .. k + 64 v + 63, then across the
waves by the same rule); a NaN or Inf candidate counts as +huge and ends the state with info = k + 1; no pivot when the
maximum is 0; info = -1 when the solution is not finite AS FLOAT32; the output is zero whenever info != 0.  It decides the
info codes and stands in for the device in the checks of this file; it is no bit-level model of the arithmetic (the kernels'
updates may contract into an fma), so only the exactly representable systems are compared to the bit.

The cases (`cases`), every one with S exact in float32:
  exact     I - S = P D, D a diagonal of powers of two in 2^-10 .. 2^10, w dyadic: x and Z are exact, compared bit for bit.
            P: the reversal; the cyclic shift that puts the pivot of every column into the LAST remaining row (n - 1
            exchanges, found by the highest active lane and wave); a seeded random permutation.
  dense     I - S = A, A standard normal rounded so that S is float32, w normal; A and A^T (the adjoint passes the
            transpose).  Seed 7000 + n for n >= 64 (61 .. 506 exchanges, cond 8e1 .. 2.6e3), 7008 and 7005 for n = 2 and 4
            (7000 + n exchanges nothing there).  Asserted from scipy: >= n / 2 exchanges for n >= 64, >= 1 for n = 2, 4.
  model     S of reduced64 at y0 of make_model(N, H, B) with Wa x 3 and m = 1 on the moving genes, for (96, 56, 4),
            (70, 97, 3), (200, 200, 2); S and S^T.  Measured with scipy: (96, 56, 4) exchanges 48 .. 60 (40 .. 50) rows in
            every state, but (70, 97, 3) only (4, 0, 0) and (200, 200, 2) none (max |S| 0.72 and 0.36: still diagonally
            dominant at y0), so "at least one exchange per state" cannot hold there: it is asserted for the first shape,
            "at least one" for the second, and per state for every shape of
  model x8  the same three shapes with Wa x 8, where every state exchanges 73 .. 222 rows.
  n in SIZES = 2, 4, 64, 66, 128, 130, 194, 512 (H = 1, 2, 32, 33, 64, 65, 97, 256): one lane, exactly one wave of pivot
  candidates, one candidate past a wave, two waves and one past, the shape of the (70, 97) tests, the largest H.
  float range  the upper bidiagonal I - S with diagonal 2^-24 and superdiagonal -2^100 at n = 6 (w = 1: x = 7.3e193, 3.4e156,
            1.6e119, 7.6e81, 3.6e44, 1.7e7 in double) and the same in the last six rows of an n = 130 identity: info = -1.

Truth and bar, nothing measured from the device: np.linalg.solve / inv in float64 of the float32 inputs; the inverse under
inverse64 of tests/test_steady_response_gpu.py as it stands; the solve by the same argument, |dA| <= gamma64_3n |L| |U| (Higham,
Theorem 9.4; L, U from scipy):   |x - x64| <= u |x64| + 2 |Z| (E |x64|),  u = 2^-24.  At n = 512 the double part is about 1e4
times the float rounding and the bar at most 5.5e-4 of its |x| (1.4e-6 in the median): far below any structural error, as
the mutations below show.

The mutations of the mirror, one at a time: the right-hand side is not swapped; the swap starts at column k + 1; the pivot
search stops after the first 64 candidates; the cross-wave reduction keeps wave 0's candidate (with candidate i = k + tid
these two choose the same pivot, the largest of the first 64).  Each one fails a named class's own assertion."""
import collections

import numpy as np
import pytest
import scipy.linalg
import torch

from test_steady_cpu import make_model, moving
from test_steady_response_gpu import gamma, inverse64, reduced64

U = 2.0 ** -24
U64 = 2.0 ** -53
SIZES = (2, 4, 64, 66, 128, 130, 194, 512)
DENSE_SEEDS = {2: 7008, 4: 7005}                          # 7000 + n elsewhere
MODEL_SHAPES = ((96, 56, 4), (70, 97, 3), (200, 200, 2))
END_TO_END = (70, 97, 3)
Y_RANGE = (-4.0, 6.0)                                     # the states of the end-to-end shape lie inside (-3.5 .. 5.2)
MUTATIONS = ("rhs not swapped", "swap from k + 1", "first 64 candidates", "wave 0's candidate")

Case = collections.namedtuple("Case", "cls n name S w")   # S [n, n], w [n] float32


# --------------------------------------------------------------------------- the mirror of the documented algorithm
def mirror(S, w, mutate=None):
    """(x [n] float32, Z [n, n] float32, info_x, info_Z, exchanges): the solve and the inverse of I - S by the documented LU,
    on the right-hand sides [w | I] at once (a column's arithmetic does not depend on its neighbours)"""
    n = len(S)
    A = np.eye(n) - S.astype(np.float64)
    R = np.concatenate([w.astype(np.float64)[:, None], np.eye(n)], axis=1)
    zero_x, zero_Z = np.zeros(n, np.float32), np.zeros((n, n), np.float32)
    swaps = 0
    with np.errstate(all="ignore"):
        for k in range(n):
            v = np.abs(A[k:, k])
            v = np.where(np.isfinite(v), v, np.inf)
            if mutate == "first 64 candidates":
                v = v[:64]
            waves = [(v[s:s + 64].max(), s + int(np.argmax(v[s:s + 64]))) for s in range(0, len(v), 64)]     # argmax: the first
            pmax, off = waves[0]
            if mutate != "wave 0's candidate":
                for val, at in waves[1:]:
                    if val > pmax:
                        pmax, off = val, at
            if not pmax > 0 or pmax == np.inf:
                return zero_x, zero_Z, k + 1, k + 1, swaps
            piv = k + off
            if piv != k:
                swaps += 1
                c0 = k + 1 if mutate == "swap from k + 1" else k
                A[[k, piv], c0:] = A[[piv, k], c0:]
                if mutate != "rhs not swapped":
                    R[[k, piv]] = R[[piv, k]]
            l = A[k + 1:, k] / A[k, k]
            R[k + 1:] -= l[:, None] * R[k][None, :]
            A[k + 1:, k + 1:] -= l[:, None] * A[k, k + 1:][None, :]
        for k in range(n - 1, -1, -1):
            R[k] /= A[k, k]
            R[:k] -= A[:k, k][:, None] * R[k][None, :]
        x, Z = R[:, 0].astype(np.float32), R[:, 1:].astype(np.float32)
    info_x = 0 if np.isfinite(x).all() else -1
    info_Z = 0 if np.isfinite(Z).all() else -1
    return (zero_x if info_x else x), (zero_Z if info_Z else Z), info_x, info_Z, swaps


def exchanges(S):
    """row exchanges of scipy's LU of I - S (LAPACK getrf: the same pivot rule)"""
    piv = scipy.linalg.lu_factor(np.eye(len(S)) - S.astype(np.float64))[1]
    return int((piv != np.arange(len(S))).sum())


# --------------------------------------------------------------------------- the cases
def permutation(kind, n):
    """perm[j]: the row that holds the only non-zero of column j"""
    if kind == "reversal":
        return np.arange(n)[::-1].copy()
    if kind == "cyclic":                                   # A[n - 1, 0], A[j - 1, j]: always the last remaining row
        return (np.arange(n) - 1) % n
    return np.random.default_rng(5000 + n).permutation(n)


def exact_system(kind, n, zero_column=None):
    """(S, w float32; x, Z exact float32) of I - S = P D"""
    rng = np.random.default_rng(6000 + n)
    perm = permutation(kind, n)
    D = 2.0 ** rng.integers(-10, 11, n)
    w = rng.integers(1, 65, n) * rng.choice([-1.0, 1.0], n) / 8
    x = w[perm] / D
    if zero_column is not None:
        D[zero_column] = 0.0
    A = np.zeros((n, n))
    A[perm, np.arange(n)] = D
    S = (np.eye(n) - A).astype(np.float32)
    assert np.array_equal(np.eye(n) - S.astype(np.float64), A) and np.array_equal(x.astype(np.float32), x)
    Z = np.zeros((n, n))
    if zero_column is None:
        Z[np.arange(n), perm] = 1 / D
    return S, w.astype(np.float32), x.astype(np.float32), Z.astype(np.float32)


def dense_system(n):
    rng = np.random.default_rng(DENSE_SEEDS.get(n, 7000 + n))
    S = (np.eye(n) - rng.standard_normal((n, n))).astype(np.float32)
    return S, rng.standard_normal(n).astype(np.float32)


def strong_model(N, H, B, factor=3):
    """make_model with Wa x factor: (p, y0, held)"""
    p, y0, held = make_model(N, H, B)
    p = dict(p, Wa=p["Wa"] * np.float32(factor))
    return p, y0, held


def model_systems(N, H, B, factor):
    p, y0, held = strong_model(N, H, B, factor)
    S = reduced64(p, y0, moving(p, held, B).astype(np.float32)).astype(np.float32)
    w = np.random.default_rng(8000 + N).standard_normal((B, 2 * H)).astype(np.float32)
    return S, w


def float_range_system(n):
    A = np.eye(n)
    for i in range(n - 6, n):
        A[i, i] = 2.0 ** -24
        if i + 1 < n:
            A[i, i + 1] = -2.0 ** 100
    S = (np.eye(n) - A).astype(np.float32)
    assert np.array_equal(np.eye(n) - S.astype(np.float64), A)
    return S, np.ones(n, np.float32)


_CASES = []


def cases():
    """every system that is held to the truth and the bar, built once"""
    if not _CASES:
        for n in SIZES:
            for kind in ("reversal", "cyclic", "random"):
                S, w, _, _ = exact_system(kind, n)
                _CASES.append(Case("exact " + kind, n, "exact %s %d" % (kind, n), S, w))
            S, w = dense_system(n)
            _CASES.append(Case("dense", n, "dense %d" % n, S, w))
            _CASES.append(Case("dense T", n, "dense T %d" % n, np.ascontiguousarray(S.T), w))
        for factor, cls in ((3, "model"), (8, "model x8")):
            for N, H, B in MODEL_SHAPES:
                S, w = model_systems(N, H, B, factor)
                for b in range(B):
                    _CASES.append(Case(cls, 2 * H, "%s (%d, %d) state %d" % (cls, N, H, b), S[b], w[b]))
                    _CASES.append(Case(cls + " T", 2 * H, "%s T (%d, %d) state %d" % (cls, N, H, b), np.ascontiguousarray(S[b].T),
                                       w[b]))
    return _CASES


Truth = collections.namedtuple("Truth", "x bar_x Z bar_Z exact")
_TRUTH = {}


def truth(case):
    """float64 x, Z of the float32 inputs and the bars of the device's float results (zero bars: the exact systems)"""
    if case.name not in _TRUTH:
        n = case.n
        if case.cls.startswith("exact"):
            _, _, x, Z = exact_system(case.cls.split()[1], n)
            _TRUTH[case.name] = Truth(x.astype(np.float64), np.zeros(n), Z.astype(np.float64), np.zeros((n, n)), True)
        else:
            S, w = case.S.astype(np.float64), case.w.astype(np.float64)
            Z, bar_Z = inverse64(S[None])
            A = np.eye(n) - S
            x = np.linalg.solve(A, w)
            _, L, Um = scipy.linalg.lu(A)
            E = gamma(3 * n, U64) * (np.abs(L) @ np.abs(Um))
            bar_x = U * np.abs(x) + 2 * np.abs(Z[0]) @ (E @ np.abs(x))
            _TRUTH[case.name] = Truth(x, bar_x, Z[0], bar_Z[0], False)
    return _TRUTH[case.name]


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.int32)


def judge(case, x, Z, info_x, info_Z):
    """the assertion of a case on the float32 results of the device (or of the mirror): None where it holds, else what
    failed; and the worst error / bar of x, of Z and of Z w against x (0 for an exact system that holds)"""
    t = truth(case)
    if info_x != 0 or info_Z != 0:
        return "info %d, %d" % (info_x, info_Z), None
    if not (np.isfinite(x).all() and np.isfinite(Z).all()):
        return "not finite", None
    if t.exact:
        ok = np.array_equal(bits(x), bits(t.x)) and np.array_equal(bits(Z), bits(t.Z))
        return (None if ok else "bits"), (0.0, 0.0, 0.0)
    ex = np.abs(x.astype(np.float64) - t.x) / t.bar_x
    eZ = np.abs(Z.astype(np.float64) - t.Z) / t.bar_Z
    w = case.w.astype(np.float64)
    both = np.abs(Z.astype(np.float64) @ w - x.astype(np.float64)) / (t.bar_Z @ np.abs(w) + t.bar_x)
    worst = (float(ex.max()), float(eZ.max()), float(both.max()))
    return (None if max(worst) <= 1.0 else "error / bar %.3g %.3g %.3g" % worst), worst


# --------------------------------------------------------------------------- info codes: inputs shared with the GPU file
INFO_N = 130
ZERO_COLUMNS = (0, 1, 63, 64, INFO_N - 2, INFO_N - 1)
NON_FINITE_AT = ((100, 1), (1, 1), (0, 1), (129, 120), (120, 120), (3, 120))     # below, on, above; an early and a late column


def singular_systems():
    """[(name, S, w, k)]: P D with D[k] = 0 -- column k has no pivot"""
    return [("%s D[%d] = 0" % (kind, k),) + exact_system(kind, INFO_N, zero_column=k)[:2] + (k,)
            for kind in ("cyclic", "random") for k in ZERO_COLUMNS]


def non_finite_systems():
    """[(name, S, w)]: the dense system with one NaN, +Inf or -Inf entry of S"""
    out = []
    for value in (np.nan, np.inf, -np.inf):
        for i, j in NON_FINITE_AT:
            S, w = dense_system(INFO_N)
            S[i, j] = value
            out.append(("%s at (%d, %d)" % (value, i, j), S, w))
    return out


def neighbours():
    """[(name, S, w)] of one size: dense, singular, exact, NaN, float range, dense"""
    n = INFO_N
    d = dense_system(n)
    return [("dense",) + d, singular_systems()[3][:3], ("exact",) + exact_system("cyclic", n)[:2], non_finite_systems()[4],
            ("float range",) + float_range_system(n), ("dense T", np.ascontiguousarray(d[0].T), d[1])]


# --------------------------------------------------------------------------- the tests
def test_the_input_conditions_hold():
    """the exchange counts, from scipy alone"""
    count = collections.defaultdict(list)
    for c in cases():
        count[(c.cls, c.n)].append(exchanges(c.S))
    print({"%s %d" % k: v for k, v in count.items()})
    for n in SIZES:
        assert count[("exact cyclic", n)] == [n - 1]
        assert count[("exact reversal", n)] == [n // 2]
        for cls in ("dense", "dense T"):
            assert count[(cls, n)][0] >= (n / 2 if n >= 64 else 1), (cls, n)
    for N, H, B in MODEL_SHAPES:
        for cls in ("model x8", "model x8 T"):
            assert len(count[(cls, 2 * H)]) == B and min(count[(cls, 2 * H)]) >= 1, (cls, N, H)
    # Wa x 3 at y0: every state of (96, 56, 4) exchanges; (70, 97, 3) in its first state only, (200, 200, 2) in none
    assert min(count[("model", 112)]) >= 1 and min(count[("model T", 112)]) >= 1
    assert max(count[("model", 194)]) >= 1 and max(count[("model T", 194)]) >= 1
    for n in (6, INFO_N):
        assert exchanges(float_range_system(n)[0]) == 0
    conds = [np.linalg.cond(np.eye(c.n) - c.S.astype(np.float64)) for c in cases() if c.cls == "dense"]
    assert max(conds) < 1e4


def test_the_mirror_passes_every_case_and_counts_scipys_exchanges():
    worst = collections.defaultdict(float)
    for c in cases():
        x, Z, ix, iZ, swaps = mirror(c.S, c.w)
        assert swaps == exchanges(c.S), c.name
        failed, w = judge(c, x, Z, ix, iZ)
        assert failed is None, (c.name, failed)
        worst[(c.cls, c.n)] = max(worst[(c.cls, c.n)], *w)
    print({"%s %d" % k: "%.2e" % v for k, v in worst.items() if v > 0})
    # the bar of the solve at n = 512 against the size of x: far below a structural error
    t = truth(next(c for c in cases() if c.name == "dense 512"))
    rel = t.bar_x / np.abs(t.x)
    print("dense 512: bar / |x| median %.1e, largest %.1e; largest bar / largest |x| %.1e"
          % (np.median(rel), rel.max(), t.bar_x.max() / np.abs(t.x).max()))
    assert t.bar_x.max() <= 1e-4 * np.abs(t.x).max()


@pytest.mark.parametrize("mutation", MUTATIONS)
def test_the_bars_bite(mutation):
    """every mutation of the mirror fails the own assertion of at least one named class"""
    by_name = {c.name: c for c in cases()}

    def failed(name):
        c = by_name[name]
        return judge(c, *mirror(c.S, c.w, mutation)[:4])[0]

    if mutation == "rhs not swapped":
        for n in (2, 4, 64, 66, 130, 194):
            assert failed("dense %d" % n) and failed("dense T %d" % n) and failed("exact cyclic %d" % n), n
        for n in (64, 66, 130):                           # every entry moves beyond twice its bar
            c = by_name["dense %d" % n]
            x, Z = mirror(c.S, c.w, mutation)[:2]
            t = truth(c)
            assert np.all(np.abs(x - t.x) > 2 * t.bar_x) and np.mean(np.abs(Z - t.Z) > 2 * t.bar_Z) > 0.99, n
        assert failed("model (96, 56) state 0") and failed("model x8 T (70, 97) state 1")
    elif mutation == "swap from k + 1":
        for n in (2, 4, 64, 66, 130):
            assert failed("dense %d" % n) and failed("exact reversal %d" % n) and failed("exact random %d" % n), n
        assert failed("model (96, 56) state 0") and failed("model x8 (200, 200) state 0")
    else:
        # the pivot of a column of P D outside the first 64 candidates is never found: a zero pivot is reported
        for n in (66, 128, 130, 194):
            assert failed("exact cyclic %d" % n) and (n < 128 or failed("exact random %d" % n)), n
        assert failed("exact reversal 130")
        for n in (2, 4, 64):                              # up to one wave of candidates the mutation changes nothing
            assert failed("exact cyclic %d" % n) is None and failed("dense %d" % n) is None, n


def test_info_codes_of_the_mirror():
    for name, S, w, k in singular_systems():
        x, Z, ix, iZ, _ = mirror(S, w)
        assert ix == iZ == k + 1 and not x.any() and not Z.any(), name
    codes = {}
    for name, S, w in non_finite_systems():
        x, Z, ix, iZ, _ = mirror(S, w)
        assert ix == iZ and 1 <= ix <= INFO_N and not x.any() and not Z.any(), name
        codes[name] = ix
    print(codes)
    # in a dense system the entry has spread over its column by the step of that column, wherever it started: an early
    # code and a pivot that fails late
    assert all(code == int(name.split(", ")[1][:-1]) + 1 for name, code in codes.items()) and set(codes.values()) == {2, 121}
    kinds = [mirror(S, w)[2] for _, S, w in neighbours()]
    assert kinds[0] == kinds[2] == kinds[5] == 0 and kinds[1] > 0 and kinds[3] > 0 and kinds[4] == -1


def test_the_float_range():
    """a solution that is finite in double and not as float is reported: info = -1 and zeros"""
    for n in (6, INFO_N):
        S, w = float_range_system(n)
        x64 = np.linalg.solve(np.eye(n) - S.astype(np.float64), w.astype(np.float64))
        assert np.all(np.isfinite(x64)) and np.all(np.isfinite(np.linalg.inv(np.eye(n) - S.astype(np.float64))))
        want = [7.3e193, 3.4e156, 1.6e119, 7.6e81, 3.6e44, 1.7e7]
        assert np.allclose(x64[n - 6:], want, rtol=0.05) and np.all(x64[:n - 6] == 1)
        with np.errstate(over="ignore"):
            assert not np.isfinite(x64.astype(np.float32)).all()
        x, Z, ix, iZ, swaps = mirror(S, w)
        assert ix == iZ == -1 and swaps == 0 and not x.any() and not Z.any()


def test_steady_solve_checks_its_arguments_before_any_device_call():
    from phoenix_amd import engine
    with pytest.raises(RuntimeError, match="must live on the GPU"):
        engine.steady_solve(torch.zeros(1, 4, 4), torch.zeros(1, 4))


# --------------------------------------------------------------------------- the end-to-end shape
def test_the_end_to_end_shape_and_the_roundings_of_its_range():
    """(70, 97, 3) with Wa x 3: the reference converges on all three rows, its fixed points reach -3.5 .. 5.2 and the systems
    of the adjoint exchange rows there.  tests/test_steady_gpu.py's kernel_truth takes "at most 16 roundings in a, l, a', l'
    for y in [0, 1)"; recounted for y in Y_RANGE = [-4, 6] (s = y - 0.5, d = 1 + |s|, correctly rounded + - * /):
      s 1;  d: 1 and s's through |s| / d < 1: 2;  a = s / d: 1 and s's and d's own through factors <= 1: 3;
      a' = 1 / (d d): 2 + 2 + 1 and the division: 6;
      l' = 1 / d (s < 0): 3, or 1 / ((1 + s) (1 + 2 s)): (1 + s): 2, (1 + 2 s): 2, the product 5, the division: 6
      (s / (1 + s) and 2 s / (1 + 2 s) are < 1 for s >= 0) -- none of these depends on the range;
      l = log1pf(a): a's 3 times the condition number a / ((1 + a) log(1 + a)), which grows as a -> -1: <= 1.5 on [0, 1),
      2.64 at y = -4 (a = -9 / 11) and < 1 for a > 0, so 3 x 2.64 < 8, and log1pf's 2 ulp <= 4 u: 12.
    The largest count is 12 <= 16: the bar holds on Y_RANGE as it stands.  Checked below on a grid in float32 numpy."""
    import phoenix_amd
    N, H, B = END_TO_END
    p, y0, held = strong_model(N, H, B)
    ref = phoenix_amd.steady_states_reference(p, y0, clamp=held, tol=1e-12, max_iter=40)
    assert np.all(ref.status == 0) and np.all(ref.iterations <= 12), (ref.status, ref.iterations)
    assert Y_RANGE[0] < ref.y.min() < -3 and 5 < ref.y.max() < Y_RANGE[1]
    S = reduced64(p, ref.y.astype(np.float32), moving(p, held, B).astype(np.float32)).astype(np.float32)
    counts = [(exchanges(S[b]), exchanges(S[b].T)) for b in range(B)]
    print("steps %s, y in %.2f .. %.2f, exchanges (S, S^T) %s" % (ref.iterations.tolist(), ref.y.min(), ref.y.max(), counts))
    assert sum(c[0] for c in counts) >= 1 and sum(c[1] for c in counts) >= 1
    # the condition number of log1p on the range, and the float32 formulas against float64 on a grid
    y = np.linspace(Y_RANGE[0], Y_RANGE[1], 200001).astype(np.float32)
    a64, l64, da64, dl64 = _acts64(y)
    far = np.abs(a64) > 1e-3
    cond = np.abs(a64[far] / ((1 + a64[far]) * np.log1p(a64[far])))
    assert cond.max() <= 2.64
    s = y - np.float32(0.5)
    d = np.float32(1) + np.abs(s)
    a = s / d
    with np.errstate(divide="ignore", invalid="ignore"):
        dl = np.where(s < 0, np.float32(1) / d, np.float32(1) / ((np.float32(1) + s) * (np.float32(1) + np.float32(2) * s)))
    got = {"a": a, "l": np.log1p(a), "a'": np.float32(1) / (d * d), "l'": dl}
    for name, ref64 in (("a", a64), ("l", l64), ("a'", da64), ("l'", dl64)):
        ok = ref64 != 0
        rel = np.abs(got[name].astype(np.float64) - ref64)[ok] / np.abs(ref64[ok]) / U
        print("%s: %.2f roundings at most on the grid" % (name, rel.max()))
        assert rel.max() <= 12, name


def _acts64(y):
    s = y.astype(np.float64) - 0.5
    d = 1 + np.abs(s)
    a = s / d
    return a, np.log1p(a), 1 / (d * d), 1 / (d * d) / (1 + a)
