"""CPU-only checks of the matrix-free products with the inferred network (phx_effects_apply /
phx_effects_apply_workspace_bytes, include/phoenix_hip.h; `effects_apply`, `network_propagation`, `propagation_reference`):
`apply_ref`, the float64 restatement on a dense matrix that tests/test_apply_gpu.py holds the kernel to, is built on the
eligibility of `neighbors_ref` (tests/test_neighbors_cpu.py) and pinned here to a brute-force double loop;
`propagation_reference` is pinned to the closed form of the walk's fixed point; the symbols exist, and the argument checks
answer before any device call."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

from test_abi_cpu import _declared_symbols
from test_neighbors_cpu import neighbors_ref

BAD_ARG, WORKSPACE = 4, 5
ORIENT, DIAGONAL = 1, 2
OF_REGULATOR, OF_TARGET = 0, 1
VALUE, ABS, UNIT = 0, 1, 2


def weights_of(value, weight):
    value = np.asarray(value, np.float64)
    return {"value": value, "abs": np.abs(value), "unit": np.ones_like(value)}[weight]


def apply_ref(M, V, of="target", weight="value", regulators=None, targets=None, threshold=None, orient=False, diagonal=False):
    """(out float64 [N, R], scale float64 [N, R], count int64 [N]) of the float32 matrix M [N, N] (regulator row, target column)
    and the block V [N, R]: out[n, r] = sum over the eligible entries of line n -- column n (of="target") or row n
    (of="regulator"), eligible as `neighbors_ref` has it -- of w(entry) V[other gene, r], w the entry, its magnitude or 1, in
    float64; scale is the same sum of |w| |V|, the quantity the rounding bound of a float32 dot product multiplies; count
    is the number of eligible entries of the line."""
    return apply_lists(lines_of(M, of=of, regulators=regulators, targets=targets, threshold=threshold, orient=orient,
                                diagonal=diagonal), V, weight)


def lines_of(M, **selection):
    """(gene [N, N], value [N, N], count [N]) of `neighbors_ref` with k = N: every line's eligible entries"""
    return neighbors_ref(np.asarray(M), np.asarray(M).shape[0], **selection)[:3]


def apply_lists(lists, V, weight):
    """`apply_ref` on the lists of `lines_of` (which do not depend on V or on the weight)"""
    gene, value, count = lists
    N = len(count)
    V = np.asarray(V, np.float64).reshape(N, -1)
    out = np.zeros(V.shape)
    scale = np.zeros(V.shape)
    for n in range(N):
        c = count[n]
        if c:
            w = weights_of(value[n, :c], weight)[:, None]
            with np.errstate(invalid="ignore"):
                out[n] = (w * V[gene[n, :c]]).sum(axis=0)
                scale[n] = (np.abs(w) * np.abs(V[gene[n, :c]])).sum(axis=0)
    return out, scale, count


def brute_force(M, V, of, weight, regulators, targets, threshold, orient, diagonal):
    """the definition, entry by entry in plain Python"""
    N, R = V.shape
    out = np.zeros((N, R))
    for n in range(N):
        for o in range(N):
            i, j = (o, n) if of == "target" else (n, o)
            a, b = float(M[i, j]), float(M[j, i])
            if not np.isfinite(a) or a == 0:
                continue
            if orient:
                if i == j or np.isnan(b) or not abs(a) > abs(b):
                    continue
            elif i == j and not diagonal:
                continue
            if regulators is not None and i not in regulators:
                continue
            if targets is not None and j not in targets:
                continue
            if threshold is not None and not abs(a) >= threshold:
                continue
            w = a if weight == "value" else (abs(a) if weight == "abs" else 1.0)
            for r in range(R):
                out[n, r] += w * float(V[o, r])
    return out


def nine_genes():
    """a 9-gene matrix with a tie pair, a NaN, an Inf, a zero column and a diagonal entry"""
    rng = np.random.default_rng(9)
    M = (rng.integers(-6, 7, size=(9, 9)) / 4.0).astype(np.float32)
    M[1, 2], M[2, 1] = 0.75, -0.75          # a tie: `orient` drops both directions
    M[3, 5] = np.nan
    M[6, 0] = np.inf
    M[:, 4] = 0.0                           # nothing regulates gene 4
    M[7, 7] = 1.25
    return M


# --------------------------------------------------------------------------- the restatement against the definition
def test_apply_ref_equals_a_brute_force_double_loop():
    M = nine_genes()
    N = M.shape[0]
    assert abs(M[1, 2]) == abs(M[2, 1]) and np.isnan(M[3, 5]) and np.isinf(M[6, 0]) and not M[:, 4].any() and M[7, 7] != 0
    rng = np.random.default_rng(1)
    V = rng.integers(-8, 9, size=(N, 3)).astype(np.float64) / 2.0            # sums of dyadic numbers: exact in any order
    cases = 0
    for of in ("target", "regulator"):
        for weight in ("value", "abs", "unit"):
            for orient in (False, True):
                for diagonal in (False, True):
                    for regulators, targets in ((None, None), ([0, 1, 2, 3, 6, 7], None), (None, [0, 2, 4, 5, 7]),
                                                ([1, 2, 7, 7], [1, 2, 7])):
                        for threshold in (None, 0.75, 0.8):
                            kw = dict(of=of, weight=weight, regulators=regulators, targets=targets, threshold=threshold,
                                      orient=orient, diagonal=diagonal)
                            out, scale, count = apply_ref(M, V, **kw)
                            want = brute_force(M, V, **kw)
                            assert np.array_equal(out, want), kw
                            assert np.all(np.isfinite(out)) and np.all(out[count == 0] == 0) and np.all(scale >= np.abs(out))
                            cases += 1
    # the zero column has no regulator; the diagonal entry counts only when it is asked for; the tie pair falls under orient
    assert apply_ref(M, V, of="target", weight="unit")[2][4] == 0
    ones = np.ones((N, 1))
    assert apply_ref(M, ones, of="target", weight="unit", diagonal=True)[0][7, 0] == \
        apply_ref(M, ones, of="target", weight="unit")[0][7, 0] + 1
    plain, oriented = apply_ref(M, ones, weight="unit", regulators=[1], targets=[2]), \
        apply_ref(M, ones, weight="unit", regulators=[1], targets=[2], orient=True)
    assert plain[0][2, 0] == 1 and oriented[0][2, 0] == 0
    # a NaN of V is seen by exactly the lines with an eligible entry at its gene
    Vn = V.copy()
    Vn[3] = np.nan
    out = apply_ref(M, Vn, of="target", weight="abs")[0]
    hit = np.array([np.isfinite(M[3, j]) and M[3, j] != 0 and j != 3 for j in range(N)])
    assert np.array_equal(np.isnan(out[:, 0]), hit) and hit.any() and not hit.all()
    print("apply_ref equals the brute-force loop in %d cases" % cases)


# --------------------------------------------------------------------------- the walk against its closed form
def six_genes():
    """regulator -> target weights of a hand-built 6-gene network; gene 5 regulates nobody (a dangling gene)"""
    M = np.zeros((6, 6), np.float32)
    for i, j, w in ((0, 1, 2.0), (0, 2, -1.0), (1, 2, 0.5), (1, 3, 1.5), (2, 0, -3.0), (2, 5, 1.0), (3, 4, 0.25), (3, 5, -0.75),
                    (4, 0, 1.0), (4, 3, 2.0), (0, 0, 9.0)):
        M[i, j] = w
    return M


def closed_form(M, p0, restart, direction, weight):
    """restart (I - (1 - restart) W~)^-1 p0, column by column: W~ is the column-stochastic walk matrix with the columns of the
    dangling genes replaced by p0"""
    A = np.abs(M).astype(np.float64) if weight == "abs" else (M != 0).astype(np.float64)
    np.fill_diagonal(A, 0.0)
    if direction == "upstream":
        A = A.T
    N = A.shape[0]
    s = A.sum(axis=1)                                        # what gene i hands out
    out = np.zeros(p0.shape)
    for r in range(p0.shape[1]):
        Wt = np.zeros((N, N))
        for i in range(N):
            Wt[:, i] = A[i, :] / s[i] if s[i] > 0 else p0[:, r]
        assert np.allclose(Wt.sum(axis=0), 1.0)
        out[:, r] = restart * np.linalg.solve(np.eye(N) - (1.0 - restart) * Wt, p0[:, r])
    return out


def test_propagation_reference_equals_the_closed_form():
    import phoenix_amd
    from phoenix_amd.analysis import propagation_steps
    M = six_genes()
    assert not M[5].any() and M[:, 5].any()                  # gene 5 dangles downstream and is reached
    seeds = np.array([[1, 0], [0, 0], [0, 3], [0, 0], [0, 1], [0, 0]], np.float64)
    p0 = seeds / seeds.sum(axis=0)
    worst = 0.0
    for direction in ("downstream", "upstream"):
        for weight in ("abs", "unit"):
            for restart, tol in ((0.5, 1e-13), (0.15, 1e-13), (0.85, 1e-13)):
                res = phoenix_amd.propagation_reference(M, torch.from_numpy(seeds), restart=restart, direction=direction,
                                                        weight=weight, tol=tol)
                want = closed_form(M, p0, restart, direction, weight)
                steps = int(np.ceil(np.log(tol / 2) / np.log(1 - restart)))
                assert res.iterations == steps == propagation_steps(restart, tol)
                assert res.score.shape == (6, 2) and res.score.dtype == np.float64 and res.residual.shape == (2,)
                err = float(np.abs(res.score - want).max())
                worst = max(worst, err)
                assert err <= 1e-12, (direction, weight, restart, err)
                assert np.all(np.abs(res.score.sum(axis=0) - 1.0) <= 1e-12) and np.all(res.score >= 0)
                assert np.all(res.residual <= tol), res.residual
    print("propagation_reference against the closed form: largest difference %.3e" % worst)
    # restart 0.5 and the default tolerance: 21 steps; a given count is taken as it is
    assert phoenix_amd.propagation_reference(M).iterations == 21 == propagation_steps(0.5, 1e-6)
    assert phoenix_amd.propagation_reference(M, iterations=3).iterations == 3
    # a list of genes is the uniform distribution over them; one column comes back as a vector
    a = phoenix_amd.propagation_reference(M, [0, 4, 4], tol=1e-13)
    b = phoenix_amd.propagation_reference(M, torch.tensor([2.0, 0, 0, 0, 2.0, 0]), tol=1e-13)
    assert a.score.shape == (6,) and np.array_equal(a.score, b.score) and np.ndim(a.residual) == 0
    want = closed_form(M, np.array([[0.5, 0, 0, 0, 0.5, 0]]).T, 0.5, "downstream", "abs")[:, 0]
    assert np.abs(a.score - want).max() <= 1e-12
    # uniform seeds
    u = phoenix_amd.propagation_reference(M, restart=0.15, tol=1e-13)
    assert np.abs(u.score - closed_form(M, np.full((6, 1), 1 / 6), 0.15, "downstream", "abs")[:, 0]).max() <= 1e-12
    # the selection arguments are those of the other analyses: without the edges into gene 5 nothing dangles any more
    t = phoenix_amd.propagation_reference(M, [0], targets=[0, 1, 2, 3, 4], tol=1e-13)
    M2 = M.copy()
    M2[:, 5] = 0
    M2[5, :] = 0
    assert t.score[5] == 0 and np.abs(t.score - closed_form(M2, np.eye(6)[:, :1], 0.5, "downstream", "abs")[:, 0]).max() <= 1e-12


# --------------------------------------------------------------------------- the C boundary
def _lib():
    from phoenix_amd import _lib
    return _lib, _lib.load()


def test_both_symbols_are_exported_and_declared():
    mod, lib = _lib()
    for name in ("phx_effects_apply_workspace_bytes", "phx_effects_apply"):
        assert name in mod.EXPORTS and name in _declared_symbols() and hasattr(lib, name), name
    assert set(mod.EXPORTS) == set(_declared_symbols())
    assert lib.phx_abi_version() == 7       # an additive change
    assert mod.APPLY_WEIGHTS == {"value": VALUE, "abs": ABS, "unit": UNIT} and mod.APPLY_MAX_R == 32
    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "phoenix_hip.h")).read()
    assert "enum phx_apply_weight { PHX_APPLY_VALUE = 0, PHX_APPLY_ABS = 1, PHX_APPLY_UNIT = 2 };" in header
    import phoenix_amd
    for name in ("effects_apply", "network_propagation", "propagation_reference", "Propagation"):
        assert getattr(phoenix_amd, name) is getattr(phoenix_amd.analysis, name)
    assert phoenix_amd.Propagation._fields == ("score", "iterations", "residual")


def test_the_unit_is_listed_and_its_listing_exists():
    from phoenix_amd import build
    assert "phx_apply.hip" in build.LISTINGS
    src = [s for s in build.sources() if os.path.basename(s) == "phx_apply.hip"]
    assert len(src) == 1 and os.path.exists(build.listing_of(src[0]))


def _params(mod, N=8, H=3, **null):
    """phx_params with made-up device addresses"""
    addr = {"Ws": 0x1000, "bs": 0x2000, "Wp": 0x3000, "bp": 0x4000, "WaT": 0x5000, "g": 0x6000}
    addr.update(null)
    return mod.PhxParams(addr["Ws"], addr["bs"], addr["Wp"], addr["bp"], addr["WaT"], addr["g"], N, H, None)


def _call(mod, lib, p="default", mode=2, y=0x7000, ph=0x8000, B=3, flags=ORIENT, axis=OF_TARGET, weight=ABS, tau=0.5, rok=0x9000,
          tok=None, V=0xa000, R=5, out=0xb000, ws=0xe000, ws_bytes=1 << 30):
    """phx_effects_apply with made-up device addresses: only calls that must return before touching the device"""
    if p == "default":
        p = _params(mod)
    return lib.phx_effects_apply(None if p is None else C.byref(p), mode, y, ph, B, flags, axis, weight, tau, rok, tok, V, R, out,
                                 ws, ws_bytes, None)


def test_bad_arguments_are_rejected_without_a_gpu():
    mod, lib = _lib()
    assert _call(mod, lib, p=None) == BAD_ARG
    for name in ("Ws", "Wp", "WaT", "g"):
        assert _call(mod, lib, p=_params(mod, **{name: None})) == BAD_ARG, name
    for bad in (dict(N=1), dict(N=0), dict(N=-8), dict(N=65536), dict(H=0), dict(H=257), dict(H=-1)):
        assert _call(mod, lib, p=_params(mod, **bad)) == BAD_ARG, bad
    for mode in (-1, 3, 7):
        assert _call(mod, lib, mode=mode) == BAD_ARG, mode
    for mode in (1, 2):                                    # the Jacobian modes need their states
        for bad in (dict(y=None), dict(ph=None), dict(B=0), dict(B=-2)):
            assert _call(mod, lib, mode=mode, **bad) == BAD_ARG, bad
    for flags in (-1, 4, 8, 7):
        assert _call(mod, lib, flags=flags) == BAD_ARG, flags
    for axis in (-1, 2, 5):
        assert _call(mod, lib, axis=axis) == BAD_ARG, axis
    for weight in (-1, 3, 17):
        assert _call(mod, lib, weight=weight) == BAD_ARG, weight
    for R in (0, -1, 33, 1000):
        assert _call(mod, lib, R=R) == BAD_ARG, R
    for tau in (-0.0, -1.0, float("inf"), float("-inf"), float("nan"), 1e39):
        assert _call(mod, lib, tau=tau) == BAD_ARG, tau
    for name in ("V", "out"):
        assert _call(mod, lib, **{name: None}) == BAD_ARG, name
    # every argument in order: the workspace is asked for next (tau = +0 is "no threshold", a subnormal is positive)
    need = lib.phx_effects_apply_workspace_bytes(8, 3, 3, 2, OF_TARGET, 5)
    assert need > 0
    for kw in (dict(), dict(tau=0.0), dict(tau=1e-45), dict(R=1), dict(R=32), dict(axis=OF_REGULATOR), dict(rok=None),
               dict(flags=0), dict(weight=VALUE), dict(weight=UNIT), dict(mode=0, y=None, ph=None, B=0)):
        assert _call(mod, lib, ws=None, **kw) == WORKSPACE, kw
    assert _call(mod, lib, ws_bytes=need - 1) == WORKSPACE
    assert _call(mod, lib, R=32, ws_bytes=need) == WORKSPACE                  # the partial blocks grow with R


def test_workspace_bytes(monkeypatch):
    _, lib = _lib()
    f = lib.phx_effects_apply_workspace_bytes
    assert f.restype is C.c_size_t
    monkeypatch.delenv("PHX_NEIGHBORS_SEGMENTS", raising=False)
    for args in ((1, 40, 3, 2, 1, 5), (0, 40, 3, 2, 1, 5), (65536, 40, 3, 2, 1, 5), (350, 0, 3, 2, 1, 5), (350, 257, 3, 2, 1, 5),
                 (350, 40, 0, 2, 1, 5), (350, 40, 0, 1, 1, 5), (350, 40, 3, 5, 1, 5), (350, 40, 3, -1, 1, 5), (350, 40, 3, 2, 2, 5),
                 (350, 40, 3, 2, -1, 5), (350, 40, 3, 2, 1, 0), (350, 40, 3, 2, 1, 33), (350, 40, 3, 2, 1, -4)):
        assert f(*args) == 0, args
    for H in (1, 40, 224, 225, 256):                       # R = 32 is served at every H, whatever the image takes of the LDS
        for mode in (0, 1, 2):
            for axis in (0, 1):
                for R in (1, 8, 32):
                    assert f(11165, H, 60, mode, axis, R) > 0, (H, mode, axis, R)
    # S partial blocks of 64-gene line tiles, R floats per line: 130 genes are 3 tiles, one segment each
    assert f(130, 40, 2, 2, 1, 5) == 3 * 192 * 5 * 4
    assert f(350, 40, 0, 0, 1, 5) == f(350, 40, -7, 0, 0, 5) > 0                             # effects ignores B
    sizes = []
    for s in ("1", "2", "3", "100"):
        monkeypatch.setenv("PHX_NEIGHBORS_SEGMENTS", s)
        sizes.append(f(130, 40, 2, 2, 1, 5))
    assert sizes == [192 * 5 * 4, 2 * 192 * 5 * 4, 3 * 192 * 5 * 4, 3 * 192 * 5 * 4]         # at most one segment per tile
    monkeypatch.delenv("PHX_NEIGHBORS_SEGMENTS")
    assert f(11165, 40, 60, 2, 1, 32) == 6 * 11200 * 32 * 4                                  # ceil(1024 / 175) segments


# --------------------------------------------------------------------------- the Python callers
def test_python_callers_refuse_bad_arguments_and_a_cpu_network():
    import phoenix_amd
    net = phoenix_amd.ODENet("cpu", 16, neurons=4)
    y = torch.rand(3, 16)
    v = torch.rand(16, 2)
    for kw in (dict(of="targets"), dict(of="row"), dict(of=None), dict(of=1),
               dict(weight="signed"), dict(weight=None), dict(weight=2), dict(weight="Abs"),
               dict(regulators=[0, 16]), dict(regulators=[-1]), dict(targets=[3, 99]), dict(targets=np.array([16])),
               dict(regulators=[0.5, 1.0]), dict(targets=[[1, 2]]), dict(regulators="abc"),
               dict(threshold=0.0), dict(threshold=-1.0), dict(threshold=float("inf")), dict(threshold=float("nan")),
               dict(threshold="1"), dict(threshold=True)):
        with pytest.raises(ValueError, match="effects_apply"):
            phoenix_amd.effects_apply(net, v, **kw)
        with pytest.raises(ValueError, match="effects_apply"):
            phoenix_amd.effects_apply(net, v, y=y, **kw)
    for bad in (torch.rand(15), torch.rand(16, 0), torch.rand(2, 16), torch.rand(16, 2, 2), [1.0] * 16, None):
        with pytest.raises(ValueError, match="effects_apply"):
            phoenix_amd.effects_apply(net, bad)
    for reduce in ("sum", "abs", None, "effects", 1):
        with pytest.raises(ValueError, match="reduce"):
            phoenix_amd.effects_apply(net, v, y=y, reduce=reduce)
    for kw in (dict(), dict(of="regulator", weight="unit"), dict(regulators=[1, 1, 2], targets=torch.tensor([0, 15])),
               dict(threshold=0.1), dict(y=y), dict(orient=True, diagonal=True), dict(weight="abs")):
        with pytest.raises(RuntimeError, match="must live on the GPU"):
            phoenix_amd.effects_apply(net, v, **kw)
        with pytest.raises(RuntimeError, match="must live on the GPU"):
            phoenix_amd.effects_apply(net, v[:, 0], **kw)

    for kw in (dict(weight="value"), dict(weight="signed"), dict(direction="down"), dict(direction=None),
               dict(restart=0.0), dict(restart=1.0), dict(restart=-0.1), dict(restart="0.5"), dict(restart=True),
               dict(tol=0.0), dict(tol=-1e-6), dict(tol="1e-6"), dict(iterations=0), dict(iterations=2.5), dict(iterations=True),
               dict(seeds=[]), dict(seeds=[16]), dict(seeds=[-1, 2]), dict(seeds=torch.zeros(16)), dict(seeds=torch.rand(15)),
               dict(seeds=torch.rand(16, 2, 1)), dict(seeds=-torch.rand(16)), dict(seeds=torch.tensor([[1.0, 0.0]] * 16)),
               dict(seeds=torch.full((16,), float("nan"))), dict(seeds="abc"), dict(seeds=[True, False]),
               dict(regulators=[16]), dict(targets=[-1]), dict(threshold=0.0)):
        with pytest.raises(ValueError, match="network_propagation"):
            phoenix_amd.network_propagation(net, **kw)
        with pytest.raises(ValueError, match="propagation_reference"):
            phoenix_amd.propagation_reference(np.eye(16, dtype=np.float32), **kw)
    for reduce in ("sum", None):
        with pytest.raises(ValueError, match="network_propagation: reduce"):
            phoenix_amd.network_propagation(net, y=y, reduce=reduce)
    for bad in (np.zeros((3, 4), np.float32), np.zeros(5, np.float32), np.zeros((1, 1), np.float32)):
        with pytest.raises(ValueError, match="propagation_reference"):
            phoenix_amd.propagation_reference(bad)
    for kw in (dict(), dict(seeds=[1, 2]), dict(seeds=torch.rand(16, 3), restart=0.15, direction="upstream", weight="unit"),
               dict(y=y, orient=True), dict(iterations=4, tol=1e-3, regulators=[0, 1], threshold=0.2)):
        with pytest.raises(RuntimeError, match="must live on the GPU"):
            phoenix_amd.network_propagation(net, **kw)
