"""CPU-only checks of the edge-extraction boundary (phx_effects_edges / phx_effects_edges_workspace_bytes,
include/phoenix_hip.h; `effects_edges`): `select_ref`, the numpy restatement of the selection that tests/test_edges_gpu.py
holds the kernel to, is pinned to the reference's own `make_mask` through the fixture g21_edges.npz
(tests/golden/make_golden_edges.py); the symbols exist, the argument checks answer before any device call, and the Python
caller refuses bad arguments and a CPU network."""
import ctypes as C

import numpy as np
import pytest
import torch

from conftest import load_golden, sub
from test_abi_cpu import _declared_symbols
from test_effects_cpu import closed_form, kernel_bound

BAD_ARG, WORKSPACE = 4, 5
COUNT, EMIT = 0, 1
ORIENT, DIAGONAL = 1, 2
WS_BYTES = 4096 * 4 + 64


def select_ref(M, top=None, threshold=None, orient=False, diagonal=False):
    """(regulator int64 [E], target int64 [E], value float32 [E]) selected from the float32 matrix M [N, N] (regulator row,
    target column): eligible = finite, non-zero, off the diagonal unless `diagonal`, and with `orient` |M[i,j]| > |M[j,i]|
    strictly (never the diagonal; a NaN partner fails); all with |M| >= threshold or the `top` largest in magnitude;
    sorted by magnitude descending, then i, then j (which also settles ties at the cut)."""
    assert (top is None) != (threshold is None)
    M = np.asarray(M)
    assert M.dtype == np.float32 and M.ndim == 2 and M.shape[0] == M.shape[1]
    N = M.shape[0]
    mag = np.abs(M)
    ok = np.isfinite(M) & (M != 0)
    eye = np.eye(N, dtype=bool)
    if orient:
        with np.errstate(invalid="ignore"):
            ok &= (mag > mag.T) & ~eye
    elif not diagonal:
        ok &= ~eye
    if threshold is not None:
        ok &= mag.astype(np.float64) >= float(threshold)       # (a Python float must not be rounded to float32)
    i, j = np.nonzero(ok)
    order = np.lexsort((j, i, -mag[i, j].astype(np.float64)))
    if top is not None:
        order = order[:top]
    i, j = i[order], j[order]
    return i.astype(np.int64), j.astype(np.int64), M[i, j]


def _lib():
    from phoenix_amd import _lib
    return _lib, _lib.load()


# --------------------------------------------------------------------------- the restatement against the reference
def test_select_ref_reproduces_the_reference_mask():
    g = load_golden("g21_edges")
    eff, masked = g["effects"], g["masked"]
    N = eff.shape[0]
    tiny = float(np.abs(eff[eff != 0]).min())
    i, j, v = select_ref(eff, threshold=tiny, orient=True)
    rebuilt = np.zeros_like(eff)
    rebuilt[i, j] = v
    print("G21: %d edges of %d entries, smallest magnitude %.3e" % (len(v), N * N, tiny))
    assert len(v) == int((masked != 0).sum()) > N
    assert np.array_equal(rebuilt.view(np.uint32), masked.view(np.uint32))
    # `diagonal` does not bring the diagonal back under `orient`
    i2, j2, v2 = select_ref(eff, threshold=tiny, orient=True, diagonal=True)
    assert np.array_equal(i, i2) and np.array_equal(j, j2) and np.array_equal(v, v2)
    assert np.all(np.diff(np.abs(v)) <= 0)


def test_golden_is_what_its_generator_asserts():
    g = load_golden("g21_edges")
    p, eff, masked = sub(g, "p_"), g["effects"], g["masked"]
    H, N = p["Ws"].shape
    assert (N, H) == (37, 5) and eff.dtype == masked.dtype == np.float32 and eff.shape == masked.shape == (N, N)
    assert int((p["g"] <= 0).sum()) >= 2 and np.all(eff[:, p["g"] <= 0] == 0)
    assert np.all(np.diag(masked) == 0)
    ref, A = closed_form(p, "effects")
    b = kernel_bound(H, 0, A)
    assert np.all(np.abs(eff.astype(np.float64) - ref) <= b)
    gap = np.abs(np.abs(eff.astype(np.float64)) - np.abs(eff.astype(np.float64)).T)
    off = ~np.eye(N, dtype=bool)
    close = gap[off] < 4 * np.maximum(b, b.T)[off]
    print("G21: pairs closer than four times the kernel bound: %d" % int(close.sum()))
    assert not close.any()


def test_select_ref_ties_and_non_finite_values():
    n, inf = np.nan, np.inf
    M = np.array([[9.0, 2.0, -2.0, n],
                  [2.0, 0.0, 3.0, 5.0],
                  [1.0, -3.0, -0.0, inf],
                  [4.0, 5.0, 7.0, 8.0]], np.float32)
    edges = lambda **kw: [(int(a), int(b), float(c)) for a, b, c in zip(*select_ref(M, **kw))]   # noqa: E731
    # every finite non-zero off-diagonal entry; equal magnitudes in index order; NaN, inf and both zeros never
    assert edges(threshold=1e-30) == [(3, 2, 7.0), (1, 3, 5.0), (3, 1, 5.0), (3, 0, 4.0), (1, 2, 3.0), (2, 1, -3.0),
                                      (0, 1, 2.0), (0, 2, -2.0), (1, 0, 2.0), (2, 0, 1.0)]
    assert edges(threshold=1e-30, diagonal=True)[:2] == [(0, 0, 9.0), (3, 3, 8.0)]
    assert len(edges(threshold=1e-30, diagonal=True)) == 12
    # orient: (0,1)/(1,0), (1,2)/(2,1) and (1,3)/(3,1) tie and lose both; (0,3) has a NaN partner: (3,0) loses, and so
    # does (0,3), being NaN; (2,3) is infinite: not eligible, and 7 > inf fails for (3,2)
    assert edges(threshold=1e-30, orient=True) == [(0, 2, -2.0)]
    # threshold is inclusive; top cuts ties by index and returns what there is
    assert edges(threshold=5.0) == [(3, 2, 7.0), (1, 3, 5.0), (3, 1, 5.0)]
    assert edges(top=2) == [(3, 2, 7.0), (1, 3, 5.0)]
    assert edges(top=5) == edges(threshold=1e-30)[:5]
    assert edges(top=100) == edges(threshold=1e-30)
    assert edges(top=3, orient=True) == [(0, 2, -2.0)]


# --------------------------------------------------------------------------- the C boundary
def test_both_symbols_are_exported_and_declared():
    mod, lib = _lib()
    for name in ("phx_effects_edges_workspace_bytes", "phx_effects_edges"):
        assert name in mod.EXPORTS and name in _declared_symbols() and hasattr(lib, name), name
    assert set(mod.EXPORTS) == set(_declared_symbols())
    assert lib.phx_abi_version() == 7       # an additive change
    assert (mod.EDGES_COUNT, mod.EDGES_EMIT, mod.EDGES_ORIENT, mod.EDGES_DIAGONAL, mod.EDGES_BINS) == (0, 1, 1, 2, 4096)
    import phoenix_amd
    assert phoenix_amd.effects_edges is phoenix_amd.analysis.effects_edges
    assert phoenix_amd.Edges._fields == ("regulator", "target", "value")


def _params(mod, N=8, H=3, **null):
    """phx_params with made-up device addresses"""
    addr = {"Ws": 0x1000, "bs": 0x2000, "Wp": 0x3000, "bp": 0x4000, "WaT": 0x5000, "g": 0x6000}
    addr.update(null)
    return mod.PhxParams(addr["Ws"], addr["bs"], addr["Wp"], addr["bp"], addr["WaT"], addr["g"], N, H, None)


def _call(mod, lib, p="default", mode=2, y=0x7000, ph=0x8000, B=3, flags=ORIENT, pass_=EMIT, level=0, prefix=0, tau=0.5,
          keys=0x9000, values=0xa000, capacity=16, ws=0xb000, ws_bytes=WS_BYTES):
    """phx_effects_edges with made-up device addresses: only calls that must return before touching the device"""
    if p == "default":
        p = _params(mod)
    return lib.phx_effects_edges(None if p is None else C.byref(p), mode, y, ph, B, flags, pass_, level, prefix, tau, keys,
                                 values, capacity, ws, ws_bytes, None)


def test_bad_arguments_are_rejected_without_a_gpu():
    mod, lib = _lib()
    assert _call(mod, lib, p=None) == BAD_ARG
    for name in ("Ws", "Wp", "WaT", "g"):
        for pass_ in (COUNT, EMIT):
            assert _call(mod, lib, p=_params(mod, **{name: None}), pass_=pass_) == BAD_ARG, name
    for bad in (dict(N=1), dict(N=0), dict(N=-8), dict(N=65536), dict(H=0), dict(H=257), dict(H=-1)):
        for pass_ in (COUNT, EMIT):
            assert _call(mod, lib, p=_params(mod, **bad), pass_=pass_) == BAD_ARG, bad
    for mode in (-1, 3, 7):
        assert _call(mod, lib, mode=mode) == BAD_ARG, mode
    for mode in (1, 2):                                    # the Jacobian modes need their states
        for bad in (dict(y=None), dict(ph=None), dict(B=0), dict(B=-2)):
            assert _call(mod, lib, mode=mode, **bad) == BAD_ARG, bad
    for flags in (-1, 4, 8, 7):
        assert _call(mod, lib, flags=flags) == BAD_ARG, flags
    for pass_ in (-1, 2, 5):
        assert _call(mod, lib, pass_=pass_) == BAD_ARG, pass_
    # COUNT: the level and the bin it refines
    for level in (-1, 2):
        assert _call(mod, lib, pass_=COUNT, level=level) == BAD_ARG, level
    for prefix in (0xff0, 0xfff, 4096, 2 ** 31):
        assert _call(mod, lib, pass_=COUNT, level=1, prefix=prefix) == BAD_ARG, prefix
    # EMIT: its list and its threshold, which must be positive and finite
    assert _call(mod, lib, keys=None) == BAD_ARG
    assert _call(mod, lib, values=None) == BAD_ARG
    assert _call(mod, lib, capacity=0) == BAD_ARG
    for tau in (0.0, -0.0, -1.0, float("inf"), float("-inf"), float("nan"), 1e39, 1e-50):   # the last two round to inf, 0
        assert _call(mod, lib, tau=tau) == BAD_ARG, tau
        assert _call(mod, lib, tau=tau, mode=0, y=None, ph=None, B=0) == BAD_ARG, tau
    # every argument in order: the workspace is asked for next
    assert _call(mod, lib, ws=None) == WORKSPACE
    assert _call(mod, lib, ws_bytes=WS_BYTES - 1) == WORKSPACE
    assert _call(mod, lib, pass_=COUNT, keys=None, values=None, capacity=0, tau=0.0, ws_bytes=0) == WORKSPACE
    assert _call(mod, lib, tau=1e-45, ws_bytes=0) == WORKSPACE              # a subnormal threshold is positive


def test_workspace_bytes_is_zero_for_a_refused_shape():
    _, lib = _lib()
    f = lib.phx_effects_edges_workspace_bytes
    for shape in ((1, 40, 3, 2), (0, 40, 3, 2), (-5, 40, 3, 2), (65536, 40, 3, 2), (350, 0, 3, 2), (350, 257, 3, 2),
                  (350, 40, 0, 2), (350, 40, 0, 1), (350, 40, 3, 5), (350, 40, 3, -1)):
        assert f(*shape) == 0, shape
    for shape in ((350, 40, 3, 2), (2, 1, 1, 1), (65535, 256, 1, 0), (350, 40, 0, 0), (350, 40, -7, 0)):   # effects ignores B
        assert f(*shape) == WS_BYTES, shape
    assert f.restype is C.c_size_t


# --------------------------------------------------------------------------- the Python caller
def test_python_caller_refuses_bad_arguments_and_a_cpu_network():
    import phoenix_amd
    net = phoenix_amd.ODENet("cpu", 16, neurons=4)
    y = torch.rand(3, 16)
    for kw in (dict(), dict(top=5, threshold=0.1), dict(top=0), dict(top=-3), dict(top=2.5), dict(top=True), dict(top="7"),
               dict(threshold=0.0), dict(threshold=-1.0), dict(threshold=float("inf")), dict(threshold=float("nan")),
               dict(threshold="1"), dict(top=5, max_edges=10), dict(threshold=0.1, max_edges=0),
               dict(threshold=0.1, max_edges=2.5), dict(threshold=0.1, max_edges=2 ** 32)):
        with pytest.raises(ValueError, match="effects_edges"):
            phoenix_amd.effects_edges(net, **kw)
        with pytest.raises(ValueError, match="effects_edges"):
            phoenix_amd.effects_edges(net, y=y, **kw)
    for reduce in ("sum", "abs", None, "effects", 1):
        with pytest.raises(ValueError, match="reduce"):
            phoenix_amd.effects_edges(net, top=5, y=y, reduce=reduce)
    for kw in (dict(top=5), dict(threshold=0.1), dict(threshold=0.1, max_edges=4), dict(top=5, y=y), dict(top=5, orient=True)):
        with pytest.raises(RuntimeError, match="must live on the GPU"):
            phoenix_amd.effects_edges(net, **kw)
